"""The training run (nnr_amd/run.py) on the device: fit() against the same loop written out from the pieces it drives, against the CPU oracle,
its selection / checkpoint files in a real run, and dev() / test() on the reference's own weights (tests/golden/eval_tiny_*.npz).

Every run uses the news tables and config of an eval_tiny fixture (61 news, title 8, abstract 16, history 6; the fixture's 5 dev impressions
of 20 samples) and a training corpus of 37 behaviours built here: one user with an empty history, impression lists of 1..9 non-clicks (K = 2:
both forms of the sampler), batch_size 8 -> four full batches and one of 5 per epoch."""
import functools
import os
import zipfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from golden_io import eval_fixture

pytestmark = pytest.mark.gpu
N_BEH, BATCH = 37, 8


def _config(z, **over):
    cast = {'int': int, 'float': float, 'str': str, 'bool': lambda v: v == 'True'}
    cfg = SimpleNamespace(**{k: cast[t](v) for k, v, t in zip(z['cfg_keys'], z['cfg_vals'], z['cfg_types'])})
    cfg.tie_order = str(z['tie_order'])
    vars(cfg).update(over)
    return cfg


def _model(tag, **over):
    """(z, cfg, model on the GPU): the package's Model of the fixture's config (with `over`) holding the fixture's state_dict."""
    from nnr_amd.model import Model
    z, held = eval_fixture(tag)
    cfg = _config(z, **over)
    model = Model(cfg, torch.zeros(cfg.vocabulary_size, cfg.word_embedding_dim))
    model.load_state_dict(held.state_dict(), strict=True)
    return z, cfg, model.cuda()


@functools.lru_cache(maxsize=None)
def _train_arrays(tag):
    """Host arrays of the training corpus over the fixture's news tables, and its impression lists [(click, [non-clicks])]: read only."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'eval_%s.npz' % tag))
    rng = np.random.default_rng(21)
    H = z['beh_history'].shape[1]
    counts = rng.integers(1, H + 1, size=N_BEH)
    counts[11] = 0                                                          # one user without history
    hist = np.zeros((N_BEH, H), dtype=np.int32)
    for b in range(N_BEH):
        hist[b, :counts[b]] = rng.integers(1, 61, size=counts[b])
    arrays = {k: z[k] for k in z.files if k.startswith('news_')}
    arrays.update(beh_user=rng.integers(0, int(z['user_num']), size=N_BEH).astype(np.int64), beh_history=hist,
                  beh_history_mask=np.arange(H)[None, :] < counts[:, None])
    beh = [(int(rng.integers(1, 61)), rng.integers(1, 61, size=b % 9 + 1).tolist()) for b in range(N_BEH)]      # 1..9 non-clicks
    for a in arrays.values():
        a.setflags(write=False)
    return arrays, counts, beh


def _corpora(tag, z, cfg):
    from nnr_amd import evaluate as E
    from nnr_amd import run as R
    from nnr_amd.corpus import DeviceCorpus, impression_lists
    arrays, _, beh = _train_arrays(tag)
    train = DeviceCorpus(arrays, 'cuda', cfg.category_num, config=cfg)
    train.set_impressions(*impression_lists(beh))
    dev = R.Split(E.dev_corpus({k: z[k] for k in z.files}, 'cuda', cfg.category_num), z['sizes'], z['labels'])
    return train, dev


def _rank_text(ranks, sizes):
    """util.py:56-62 for given ranks: line i = '<i> [r0,r1,...]', no trailing newline."""
    r, o, lines = [int(v) for v in ranks], 0, []
    for i, n in enumerate(int(s) for s in sizes):
        lines.append('%d %s' % (i + 1, str(r[o:o + n]).replace(' ', '')))
        o += n
    return '\n'.join(lines)


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


def _hand_loop(model, cfg, train, dev, tmp, listwise=False):
    """What fit() must equal, from the pre-existing public pieces only.  -> (losses, metrics, rank-file bytes per epoch, flat parameters)."""
    from nnr_amd import dp
    from nnr_amd import evaluate as E
    from nnr_amd.trainer import Trainer
    trainer = Trainer(model, cfg)
    losses, metrics, files = [], [], []
    for e in range(1, cfg.epoch + 1):
        train.sample_negatives(e, seed=cfg.seed, negative_sample_num=cfg.negative_sample_num)
        order = dp.sampler_indices(train.num, 0, 1, e, seed=cfg.seed).cuda()
        model.train()
        total = torch.zeros((), device='cuda', dtype=torch.float64)
        for start in range(0, train.num, cfg.batch_size):
            idx = order[start:start + cfg.batch_size]
            _, loss = trainer.train_step(train.train_batch(idx))
            total += loss.reshape(()).double() * idx.numel()
        losses.append(float(total) / train.num)
        m, ranks = E.evaluate(model, dev.corpus, dev.labels, dev.sizes, cfg.batch_size * 3 // 2, listwise=listwise)
        path = os.path.join(str(tmp), 'hand-%d.txt' % e)
        E.write_result_file(path, ranks, dev.sizes.tolist())
        metrics.append(m)
        files.append(_read(path))
    torch.cuda.synchronize()
    return losses, metrics, files, trainer.flat.flat.detach().cpu().clone()


def _dev_files(dirs, run, name, epochs):
    return [_read(os.path.join(dirs.path('dev_res_dir'), '#%d' % run, '%s-%d.txt' % (name, e))) for e in range(1, epochs + 1)]


# ------------------------------------------------------------------------------------------------------------------ 1 + 5: the native, replayed step
@pytest.fixture(scope='module')
def native_run(tmp_path_factory):
    """fit() of tiny_CNE_SUE_stable for 4 epochs, and the hand-written loop on a second model built the same way."""
    from nnr_amd import run as R
    from nnr_amd.trainer import Trainer
    tag, tmp = 'tiny_CNE_SUE_stable', tmp_path_factory.mktemp('native_run')
    over = dict(batch_size=BATCH, epoch=4, early_stopping_epoch=9)
    z, cfg, model = _model(tag, **over)
    train, dev = _corpora(tag, z, cfg)
    dirs = R.RunDirs(str(tmp / 'root'), cfg.dataset, model.model_name)
    trainer, paths = Trainer(model, cfg), []
    result = R.fit(model, cfg, train, dev, dirs, trainer=trainer, on_step=lambda e, s, t: paths.append((e, s, t.last_path)), log=lambda *a: None)
    torch.cuda.synchronize()
    flat = trainer.flat.flat.detach().cpu().clone()
    _, _, twin = _model(tag, **over)
    hand = _hand_loop(twin, cfg, train, dev, tmp)
    return SimpleNamespace(tag=tag, z=z, cfg=cfg, dev=dev, dirs=dirs, result=result, paths=paths, trainer=trainer, flat=flat, hand=hand)


def test_fit_equals_the_hand_written_loop_on_the_replayed_step(native_run):
    r = native_run
    losses, metrics, files, flat = r.hand
    res = r.result
    print('paths:', r.paths)
    print('losses fit %r\n       hand %r' % (res.losses, losses))
    assert (res.epochs_run, res.run_index) == (4, 1) and 1 <= res.best_epoch <= 4
    assert res.losses == losses                                             # bit-identical: the same launches in the same order
    assert res.metrics == metrics
    assert _dev_files(r.dirs, 1, 'CNE-SUE', 4) == files
    assert torch.equal(r.flat, flat)
    # the tape of the full batches is recorded at step 3 and replays from step 4 of epoch 1 on, through every evaluation and redraw; the
    # 5-row batch is call by call in epochs 1-2, recorded in epoch 3 and replayed in epoch 4
    want = {1: ['native', 'native', 'record', 'replay', 'native'], 2: ['replay'] * 4 + ['native'], 3: ['replay'] * 4 + ['record'],
            4: ['replay'] * 5}
    assert r.paths == [(e, s, p) for e in (1, 2, 3, 4) for s, p in enumerate(want[e], 1)]
    assert r.trainer.tape_violations == [] and len(r.trainer.tapes) == 2


def test_a_checkpoint_of_the_run_is_the_model_of_that_epoch(native_run):
    """The best file in a fresh Model scores the dev split exactly as the run did in that epoch: evaluation inside the run saw the parameters
    the last replayed optimizer step wrote (no stale derived weights), and the checkpoint was taken from them."""
    from nnr_amd import evaluate as E
    from nnr_amd import run as R
    from nnr_amd.model import Model
    r, res = native_run, native_run.result
    assert res.best_model_path == os.path.join(r.dirs.path('best_model_dir'), '#1', 'CNE-SUE')
    assert _read(res.best_model_path) == _read(os.path.join(r.dirs.path('model_dir'), '#1', 'CNE-SUE-%d' % res.best_epoch))
    fresh = Model(r.cfg, torch.zeros(r.cfg.vocabulary_size, r.cfg.word_embedding_dim))
    fresh.load_state_dict(torch.load(res.best_model_path, map_location='cpu', weights_only=True)['CNE-SUE'], strict=True)
    m, ranks = E.evaluate(fresh.cuda(), r.dev.corpus, r.dev.labels, r.dev.sizes, BATCH * 3 // 2)
    assert m == res.metrics[res.best_epoch - 1]
    assert _rank_text(ranks.cpu().tolist(), r.dev.sizes).encode() == _dev_files(r.dirs, 1, 'CNE-SUE', res.best_epoch)[-1]
    # the run's other files
    assert _read(os.path.join(r.dirs.path('result_dir'), '#1-dev')).decode() == R.result_line(1, *res.metrics[res.best_epoch - 1])
    log = _read(os.path.join(r.dirs.path('dev_res_dir'), '#1', 'CNE-SUE-%s-dev_log.txt' % r.cfg.dataset)).decode()
    assert log == R.dev_log_text(res.metrics) and log.count('\n') == 5
    assert os.path.exists(os.path.join(r.dirs.path('config_dir'), '#1.json'))


# ------------------------------------------------------------------------------------------------------------------ 2: the autograd path
def _diff(a, b):
    """Largest absolute difference between two (losses, metrics, files, flat) results, per component; rank files count as 0 / inf."""
    return (max(abs(x - y) for x, y in zip(a[0], b[0])), max(abs(x - y) for m, n in zip(a[1], b[1]) for x, y in zip(m, n)),
            0.0 if a[2] == b[2] else float('inf'), float((a[3] - b[3]).abs().max()))


@pytest.fixture(scope='module')
def autograd_runs(tmp_path_factory):
    """tiny_CNN_ATT for 3 epochs: the hand-written loop twice, then fit() with listwise=False and with listwise=True, each on a model of its own."""
    from nnr_amd import evaluate as E
    from nnr_amd import run as R
    from nnr_amd.trainer import Trainer
    tag, over, tmp = 'tiny_CNN_ATT', dict(batch_size=BATCH, epoch=3, early_stopping_epoch=9), tmp_path_factory.mktemp('autograd_runs')
    z, cfg, first = _model(tag, **over)
    train, dev = _corpora(tag, z, cfg)
    hand = _hand_loop(first, cfg, train, dev, tmp)
    again = _hand_loop(_model(tag, **over)[2], cfg, train, dev, tmp)
    runs = {}
    for listwise in (False, True):
        _, _, model = _model(tag, **over)
        dirs = R.RunDirs(str(tmp / ('list' if listwise else 'plain')), cfg.dataset, model.model_name)
        trainer, paths = Trainer(model, cfg), set()
        res = R.fit(model, cfg, train, dev, dirs, trainer=trainer, listwise=listwise, on_step=lambda e, s, t: paths.add(t.last_path), log=lambda *a: None)
        torch.cuda.synchronize()
        assert paths == {'autograd'} and E.LAST_STATS['mode'] == ('listwise' if listwise else 'cached')
        runs[listwise] = SimpleNamespace(result=res, model=model, out=(res.losses, res.metrics, _dev_files(dirs, res.run_index, 'CNN-ATT', 3),
                                                                       trainer.flat.flat.detach().cpu().clone()))
    return SimpleNamespace(hand=hand, again=again, runs=runs, dev=dev)


def test_fit_equals_the_hand_written_loop_on_the_autograd_path(autograd_runs):
    """fit() must agree with the hand-written loop within what two runs of the hand-written loop differ by, component by component: zero
    wherever the existing kernels are bit-reproducible for this pair.

    Measured on an MI355X (5 runs of the loop and 5 of fit(), all 45 pairs): the per-epoch losses, the per-epoch dev metrics and every rank
    file were bit-identical in every pair.  The flat parameter buffer is NOT bit-reproducible on this path (the gradient reductions of the
    autograd step add with float atomics): 20 to 54 of its 1816 elements differed by 2.3e-10 to 3.0e-8 (1 to 8 ulp of the element) -- among
    two runs of the loop (3.7e-9 or 1.5e-8), among two runs of fit() (1.9e-9 to 3.0e-8) and between a loop and a fit() run (2.3e-10 to 3.0e-8)
    alike.  The bound on that component is therefore itself a draw from the distribution the difference under test is drawn from, and its
    assertion below holds or fails by that draw (the first GPU run of this file: 1.5e-8 against a bound of 3.7e-9, failed; the next four
    passed, one of them with 3.0e-8 against 6.0e-8); the bound is kept as set."""
    r = autograd_runs
    spread, d = _diff(r.hand, r.again), _diff(r.runs[False].out, r.hand)
    for name, s, v in zip(('losses', 'metrics', 'rank files', 'parameters'), spread, d):
        print('%-10s hand-written loop run to run %.3e, fit against the loop %.3e' % (name, s, v))
    assert r.runs[False].result.epochs_run == 3
    assert d[0] <= spread[0] and d[1] <= spread[1] and d[2] <= spread[2]
    assert d[3] <= spread[3]


def test_listwise_evaluation_in_the_run_selects_the_same_epoch(autograd_runs):
    from nnr_amd import evaluate as E
    r = autograd_runs
    plain, listed, dev = r.runs[False], r.runs[True], r.dev
    assert listed.result.best_epoch == plain.result.best_epoch and listed.result.epochs_run == 3
    bs = BATCH * 3 // 2
    scores = [E.compute_scores(plain.model, dev.corpus, bs), E.compute_scores_listwise(plain.model, dev.corpus, dev.sizes, bs),
              E.compute_scores(listed.model, dev.corpus, bs), E.compute_scores_listwise(listed.model, dev.corpus, dev.sizes, bs)]
    worst = max(float((a - scores[0]).abs().max()) for a in scores[1:])
    print('dev scores of the two runs in the two forms: max difference %.3e' % worst)
    assert worst <= 2e-6


# ------------------------------------------------------------------------------------------------------------------ 3: the CPU oracle
def test_an_epoch_against_the_cpu_oracle(tmp_path):
    from nnr_amd import dp
    from nnr_amd import run as R
    from oracle import corpus_oracle as CO, nnr_oracle as O
    tag = 'tiny_CNN_ATT'
    z, cfg, model = _model(tag, batch_size=BATCH, epoch=1, dropout_rate=0.0)
    train, dev = _corpora(tag, z, cfg)
    ref = O.Model(O.default_config(**vars(cfg)))
    ref.load_state_dict(eval_fixture(tag)[1].state_dict())
    ref.train()
    opt = O.make_optimizer(ref, cfg)
    res = R.fit(model, cfg, train, dev, R.RunDirs(str(tmp_path), cfg.dataset, model.model_name), log=lambda *a: None)
    arrays, counts, _ = _train_arrays(tag)
    c = dict(arrays, train_samples=train.samples.cpu().numpy(), beh_line=np.arange(N_BEH))     # epoch 1's table, as the device drew it
    g = [CO.history_graph(arrays['news_category'][arrays['beh_history'][b]], int(counts[b]), cfg.max_history_num, cfg.category_num) for b in range(N_BEH)]
    c.update(train_user_history_graph=np.stack([x[0] for x in g]), train_user_history_category_mask=np.stack([x[1] for x in g]),
             train_user_history_category_indices=np.stack([x[2] for x in g]))
    order = dp.sampler_indices(N_BEH, 0, 1, 1, seed=cfg.seed).numpy()
    total = 0.0
    for start in range(0, N_BEH, BATCH):
        idx = order[start:start + BATCH]
        batch = [torch.from_numpy(np.ascontiguousarray(a)) for a in CO.train_batch(c, idx)]
        total += O.train_step(ref, opt, batch, cfg.gradient_clip_norm)[1] * len(idx)
    err = abs(res.losses[0] - total / N_BEH)
    print('epoch loss %.8f, oracle %.8f: |difference| %.3e' % (res.losses[0], total / N_BEH, err))
    assert res.epochs_run == 1 and err <= 5e-5


# ------------------------------------------------------------------------------------------------------------------ 4: selection in a real run
def test_ties_count_as_improvement_in_a_real_run(tmp_path):
    from nnr_amd import run as R
    tag = 'tiny_CNN_ATT'
    z, cfg, model = _model(tag, batch_size=BATCH, epoch=4, early_stopping_epoch=2, lr=0.0)
    train, dev = _corpora(tag, z, cfg)
    dirs = R.RunDirs(str(tmp_path), cfg.dataset, model.model_name)
    res = R.fit(model, cfg, train, dev, dirs, log=lambda *a: None)
    print('metrics per epoch:', res.metrics)
    assert res.metrics[1:] == res.metrics[:-1]                              # lr = 0: the parameters never move
    assert (res.epochs_run, res.best_epoch) == (4, 4)
    models = os.path.join(dirs.path('model_dir'), '#1')
    assert sorted(os.listdir(models)) == ['CNN-ATT-%d' % e for e in (1, 2, 3, 4)]
    assert res.best_model_path == os.path.join(dirs.path('best_model_dir'), '#1', 'CNN-ATT')
    assert _read(res.best_model_path) == _read(os.path.join(models, 'CNN-ATT-4'))
    assert _read(os.path.join(dirs.path('result_dir'), '#1-dev')).decode() == R.result_line(1, *res.metrics[3])


# ------------------------------------------------------------------------------------------------------------------ 6: dev / test modes
@pytest.mark.parametrize('tag', ['tiny_CNE_SUE_stable', 'tiny_CNN_ATT', 'tiny_CNN_CATT', 'tiny_MHSA_MHSA'])
def test_dev_and_test_modes_on_the_reference_weights(tag, tmp_path):
    from nnr_amd import evaluate as E
    from nnr_amd import run as R
    from nnr_amd.model import Model
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'eval_%s.npz' % tag))
    path = str(tmp_path / 'weights')
    cfg = _config(z, batch_size=4, world_size=1, dev_model_path=path, test_model_path=path, mode='dev')     # evaluation at 8, the fixtures' batch
    new = lambda: Model(cfg, torch.zeros(cfg.vocabulary_size, cfg.word_embedding_dim))
    name = new().model_name
    torch.save({name: {k[len('state/'):]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith('state/')}}, path)
    dirs = R.RunDirs(str(tmp_path / 'root'), cfg.dataset, name)
    dc = E.dev_corpus({k: z[k] for k in z.files}, 'cuda', cfg.category_num)
    want = _rank_text(z['ranks'], z['sizes']).encode()
    sub = path.replace('\\', '_').replace('/', '_')
    got = R.dev(new(), cfg, R.Split(dc, z['sizes'], z['labels']), dirs, log=lambda *a: None)
    print('%s: metrics %r, |difference| %.3e' % (tag, got, float(np.abs(np.asarray(got) - z['metrics']).max())))
    np.testing.assert_allclose(np.asarray(got), z['metrics'], rtol=0, atol=1e-12)
    assert _read(os.path.join(dirs.path('dev_res_dir'), sub, name + '.txt')) == want
    # a test split without labels: ranks only
    cfg.mode = 'test'
    assert R.test(new(), cfg, R.Split(dc, z['sizes'], None), dirs, log=lambda *a: None) is None
    assert _read(os.path.join(dirs.path('test_res_dir'), sub, name + '.txt')) == want
    cfg.mode = 'train'
    assert R.test(new(), cfg, R.Split(dc, z['sizes'], None), dirs, run_index=2, log=lambda *a: None) is None
    assert not os.path.exists(dirs.path('result_dir'))                      # no '-test' line without labels
    pred = os.path.join(dirs.path('prediction_dir'), '#2')
    assert _read(os.path.join(pred, 'prediction.txt')) == want
    with zipfile.ZipFile(os.path.join(pred, 'prediction.zip')) as zf:
        assert zf.namelist() == ['prediction.txt'] and zf.read('prediction.txt') == want
    # with labels: the '-test' line in train mode, --test_output_file in test mode
    m = R.test(new(), cfg, R.Split(dc, z['sizes'], z['labels']), dirs, run_index=2, log=lambda *a: None)
    assert m == got and _read(os.path.join(dirs.path('result_dir'), '#2-test')).decode() == R.result_line(2, *got)
    cfg.mode, cfg.test_output_file = 'test', str(tmp_path / 'out.txt')
    R.test(new(), cfg, R.Split(dc, z['sizes'], z['labels']), dirs, log=lambda *a: None)
    assert _read(cfg.test_output_file).decode() == R.result_line(cfg.seed + 1, *got)
