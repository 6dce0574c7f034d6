"""Host side of the training run (nnr_amd/run.py): the flags it reads, AvgMetric, the selection / early-stopping bookkeeping against tables
derived by hand from the reference's trainer.py:132-185, the directory layout and file formats, the checkpoint format, and the refusals.
Nothing here launches a kernel; the run itself is tests/test_hip_run_gpu.py."""
import os
from types import SimpleNamespace

import pytest
import torch

from golden_io import eval_fixture
from nnr_amd import run as R
from nnr_amd.config import make_config


# ------------------------------------------------------------------------------------------------------------------ flags
def test_run_flags_have_the_reference_defaults():
    c = make_config([])
    assert (c.dev_model_path, c.test_model_path, c.test_output_file, c.dev_criterion, c.early_stopping_epoch) == ('', '', '', 'avg', 5)
    assert c.mode == 'train'
    for crit in ('auc', 'mrr', 'ndcg5', 'ndcg10', 'avg'):
        assert make_config(['--dev_criterion=' + crit]).dev_criterion == crit
    for mode in ('train', 'dev', 'test'):
        assert make_config(['--mode=' + mode]).mode == mode
    with pytest.raises(SystemExit):
        make_config(['--dev_criterion=bogus'])
    with pytest.raises(SystemExit):
        make_config(['--mode=bogus'])
    c = make_config(['--dev_model_path=a/b', '--test_model_path=c', '--test_output_file=out.txt', '--early_stopping_epoch=2'])
    assert (c.dev_model_path, c.test_model_path, c.test_output_file, c.early_stopping_epoch) == ('a/b', 'c', 'out.txt', 2)
    # the values tests/test_config_synth.py checks are where they were
    c = make_config([])
    assert (c.news_encoder, c.user_encoder, c.batch_size, c.lr, c.gradient_clip_norm) == ('CNE', 'SUE', 64, 1e-4, 4.0)
    assert (c.max_title_length, c.max_abstract_length, c.max_history_num, c.negative_sample_num) == (32, 128, 50, 4)
    assert (c.hidden_dim, c.attention_dim, c.head_num, c.head_dim, c.word_embedding_dim) == (200, 200, 20, 20, 300)
    assert (c.dropout_rate, c.gcn_layer_num, c.epoch) == (0.2, 4, 8)
    assert make_config(['--gcn_normalization_type=asymmetric']).gcn_normalization_type == 'asymmetric'
    with pytest.raises(SystemExit):
        make_config(['--gcn_normalization_type=bogus'])


def test_make_config_still_has_no_side_effects(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    make_config(['--mode=train', '--dev_criterion=auc'])
    assert list(tmp_path.iterdir()) == []


# ------------------------------------------------------------------------------------------------------------------ AvgMetric
def test_avg_metric():
    a = R.AvgMetric(0.6, 0.3, 0.3, 0.4)
    assert a.avg == (0.6 + 0.3 + 0.35) / 3
    assert (a.auc, a.mrr, a.ndcg5, a.ndcg10) == (0.6, 0.3, 0.3, 0.4)
    lo, same = R.AvgMetric(0.5, 0.3, 0.3, 0.4), R.AvgMetric(0.3, 0.6, 0.4, 0.3)      # `same`: other metrics, the same average
    assert same.avg == a.avg
    assert a > lo and not lo > a and not a > same
    assert a >= lo and a >= same and not lo >= a
    assert lo < a and not a < lo and not a < same
    assert lo <= a and a <= same and not a <= lo
    assert str(a) == '0.4167\nAUC = 0.6000\nMRR = 0.3000\nnDCG@5 = 0.3000\nnDCG@10 = 0.4000'
    assert R.AvgMetric(0, 0, 0, 0).avg == 0


# ------------------------------------------------------------------------------------------------------------------ Selection
# Tables derived by hand from trainer.py:132-185: the criterion's value per epoch -> (improved, best_epoch, epoch_not_increase, stop) after
# that epoch.  "improved" is value >= best (best starts at 0); the counter resets on improvement, else grows; stop is counter == patience.
TABLES = {
    'rising': (2, [0.5, 0.6, 0.7],
               [(True, 1, 0, False), (True, 2, 0, False), (True, 3, 0, False)]),
    'tie': (3, [0.6, 0.5, 0.6, 0.6],                           # an exact tie: the LATER epoch becomes best, the counter resets
            [(True, 1, 0, False), (False, 1, 1, False), (True, 3, 0, False), (True, 4, 0, False)]),
    'fall': (2, [0.7, 0.6, 0.65],                              # two epochs below the best with patience 2: stops at epoch 3, not at 4
             [(True, 1, 0, False), (False, 1, 1, False), (False, 1, 2, True)]),
    'patient': (9, [0.7, 0.6, 0.5, 0.4],                       # patience longer than the run: never stops
                [(True, 1, 0, False), (False, 1, 1, False), (False, 1, 2, False), (False, 1, 3, False)]),
    'zero': (1, [0.0, 0.0],                                    # 0 >= the initial best of 0
             [(True, 1, 0, False), (True, 2, 0, False)]),
}
POSITION = {'auc': 0, 'mrr': 1, 'ndcg5': 2, 'ndcg10': 3}


@pytest.mark.parametrize('table', sorted(TABLES))
@pytest.mark.parametrize('criterion', ['auc', 'mrr', 'ndcg5', 'ndcg10', 'avg'])
def test_selection_tables(criterion, table):
    patience, values, want = TABLES[table]
    sel = R.Selection(criterion, patience)
    assert (sel.best_epoch, sel.epoch_not_increase, sel.stop) == (0, 0, False)
    for e, (v, w) in enumerate(zip(values, want), 1):
        if criterion == 'avg':
            m = [v, v, v, v]                                   # avg = (v + v + (v + v) / 2) / 3: rises, falls and ties with v
        else:
            m = [1.0 - 0.1 * e] * 4                            # the other three metrics fall throughout: they must not be read
            m[POSITION[criterion]] = v
        improved = sel.update(e, *m)
        assert (improved, sel.best_epoch, sel.epoch_not_increase, sel.stop) == w, (criterion, table, e)


def test_selection_by_avg_reads_the_average_not_auc():
    epochs = [(0.7, 0.3, 0.3, 0.3), (0.6, 0.5, 0.4, 0.4)]      # avg 1.3 / 3 -> 1.5 / 3 while auc falls 0.7 -> 0.6
    by_avg, by_auc = R.Selection('avg', 5), R.Selection('auc', 5)
    assert [by_avg.update(e, *m) for e, m in enumerate(epochs, 1)] == [True, True]
    assert [by_auc.update(e, *m) for e, m in enumerate(epochs, 1)] == [True, False]
    assert (by_avg.best_epoch, by_avg.epoch_not_increase) == (2, 0) and (by_auc.best_epoch, by_auc.epoch_not_increase) == (1, 1)
    assert by_avg.best.avg == (0.6 + 0.5 + 0.4) / 3 and by_auc.best == 0.7
    with pytest.raises(ValueError):
        R.Selection('bogus', 5)


# ------------------------------------------------------------------------------------------------------------------ files
def test_run_index(tmp_path):
    d = str(tmp_path)
    assert R.get_run_index(d) == 1
    assert os.listdir(d) == ['#1-dev'] and os.path.getsize(os.path.join(d, '#1-dev')) == 0
    other = tmp_path / 'other'
    other.mkdir()
    for name in ('#3-dev', '#1-test', 'notes.txt'):
        (other / name).write_text('x')
    assert R.get_run_index(str(other)) == 4
    assert sorted(os.listdir(str(other))) == ['#1-test', '#3-dev', '#4-dev', 'notes.txt']
    assert (other / '#3-dev').read_text() == 'x' and (other / '#4-dev').read_text() == ''


def test_directory_layout(tmp_path):
    root = tmp_path / 'runs'
    dirs = R.RunDirs(str(root), 'small', 'CNN-ATT')
    want = dict(config_dir='configs/small/CNN-ATT', model_dir='models/small/CNN-ATT', best_model_dir='best_model/small/CNN-ATT',
                dev_res_dir='dev/res/small/CNN-ATT', test_res_dir='test/res/small/CNN-ATT', result_dir='results/small/CNN-ATT',
                prediction_dir='prediction/small/CNN-ATT')
    for name, rel in want.items():
        assert dirs.path(name) == os.path.join(str(root), *rel.split('/'))
    assert not root.exists()                                   # path() creates nothing
    assert R.RunDirs('.', 'small', 'CNN-ATT').path('best_model_dir') == os.path.join('best_model', 'small', 'CNN-ATT')     # the reference's own strings
    assert dirs.model_dir == dirs.path('model_dir') and os.path.isdir(dirs.model_dir)
    assert sorted(os.listdir(str(root))) == ['models']         # created on use, one by one
    assert dirs.run_dir('dev_res_dir', 7) == os.path.join(dirs.path('dev_res_dir'), '#7') and os.path.isdir(dirs.run_dir('dev_res_dir', 7))
    with pytest.raises(AttributeError):
        dirs.no_such_dir


def test_result_line_and_dev_log_bytes():
    m = (0.7866666666666666, 0.6333333333333333, 0.8, 0.8)
    assert R.result_line(3, *m) == '#3\t0.7866666666666666\t0.6333333333333333\t0.8\t0.8\n'
    assert R.result_line(1, 0.5, 1.0, 1e-05, 0.125) == '#1\t0.5\t1.0\t1e-05\t0.125\n'
    assert R.dev_log_text([m, (0.5, 0.25, 0.125, 1.0)]) == ('Epoch\tAUC\tMRR\tnDCG@5\tnDCG@10\n'
                                                            '1\t0.7867\t0.6333\t0.8000\t0.8000\n'
                                                            '2\t0.5000\t0.2500\t0.1250\t1.0000\n')


@pytest.mark.parametrize('flat', [False, True])
def test_checkpoint_format(tmp_path, flat):
    """flat=True: the parameters are views of one flat buffer, as after Trainer(model, ...) -- the state a run saves."""
    _, model = eval_fixture('tiny_CNN_ATT')
    if flat:
        from nnr_amd.trainer import FlatParams
        FlatParams(model)
    want = model.state_dict()
    assert any(k.startswith('user_encoder.news_encoder.') for k in want)
    state = R.checkpoint_state(model)
    live = {p.untyped_storage().data_ptr() for p in model.parameters()} | {b.untyped_storage().data_ptr() for b in model.buffers()}
    for k, v in state.items():
        assert v.device.type == 'cpu' and v.is_contiguous() and not v.requires_grad, k
        assert v.untyped_storage().data_ptr() not in live, k + ' shares storage with the model'
        assert v.untyped_storage().nbytes() == v.numel() * v.element_size(), k + ' is a view of something larger'
    path = str(tmp_path / 'CNN-ATT-1')
    R.save_checkpoint(model, path)
    assert os.path.getsize(path) < 2 * sum(p.numel() * 4 for p in model.parameters()) + (1 << 16)
    got = torch.load(path, map_location='cpu', weights_only=True)
    assert list(got) == ['CNN-ATT']
    got = got['CNN-ATT']
    assert list(got) == list(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and torch.equal(got[k], want[k].detach()), k
    _, fresh = eval_fixture('tiny_CNN_ATT')
    with torch.no_grad():
        for p in fresh.parameters():
            p.add_(1.0)
    R.load_checkpoint(fresh, path, 'Dev')                       # strict
    for (k, a), (_, b) in zip(fresh.state_dict().items(), want.items()):
        assert torch.equal(a, b), k
    with torch.no_grad():                                       # the file is a copy: later training does not reach it
        for p in model.parameters():
            p.zero_()
    assert any(float(v.abs().max()) > 0 for v in state.values())


def test_missing_model_files_raise_the_reference_text(tmp_path):
    _, model = eval_fixture('tiny_CNN_ATT')
    dirs = R.RunDirs(str(tmp_path / 'root'), 'tiny', 'CNN-ATT')
    cfg = SimpleNamespace(batch_size=4, world_size=1, dev_model_path='no/such/file', test_model_path='nor/this', mode='test')
    with pytest.raises(AssertionError, match='^Dev model does not exist : no/such/file$'):
        R.dev(model, cfg, None, dirs)
    with pytest.raises(AssertionError, match='^Test model does not exist : nor/this$'):
        R.test(model, cfg, None, dirs)
    assert not (tmp_path / 'root').exists()


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_any_file(tmp_path, monkeypatch):
    root = tmp_path / 'root'
    dirs = R.RunDirs(str(root), 'tiny', 'CNN-ATT')
    _, model = eval_fixture('tiny_CNN_ATT')
    with_lists = SimpleNamespace(sampler=object(), num=5, device='cpu')
    without = SimpleNamespace(sampler=None, num=5, device='cpu')
    base = dict(batch_size=4, epoch=2, seed=0, negative_sample_num=2, lr=1e-4, weight_decay=0.0, gradient_clip_norm=4.0, mode='train')
    with pytest.raises(NotImplementedError, match='world_size=2'):
        R.fit(model, SimpleNamespace(world_size=2, **base), with_lists, None, dirs)
    with pytest.raises(ValueError, match='impression lists'):
        R.fit(model, SimpleNamespace(world_size=1, **base), without, None, dirs)
    with pytest.raises(ValueError, match='epoch=0'):
        R.fit(model, SimpleNamespace(world_size=1, **dict(base, epoch=0)), with_lists, None, dirs)
    for fn in (R.dev, R.test):
        with pytest.raises(NotImplementedError, match='world_size=2'):
            fn(model, SimpleNamespace(world_size=2, **base), None, dirs)
    with pytest.raises(ValueError, match='run_index'):         # train mode files the test result under the run's index
        R.test(model, SimpleNamespace(world_size=1, test_model_path='x', **base), None, dirs)
    monkeypatch.setattr(R.dp, 'world_size', lambda: 2)         # an initialised process group of two ranks
    with pytest.raises(NotImplementedError, match='process group of 2'):
        R.fit(model, SimpleNamespace(world_size=1, **base), with_lists, None, dirs)
    assert not root.exists()
