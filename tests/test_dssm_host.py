"""CPU checks of the DSSM baseline (nnr_amd/dssm.py, csrc/dssm.hip): the float64 restatement tests/dssm_ref.py against the fixtures that
tools/make_dssm_goldens.py produced with the reference's own DSSM_model.DSSM, the reference's parameter names, shapes and initialisation,
the flags of DSSM_util.py:34-57, the constructor's refusals, the C-ABI plumbing and the synthetic tf-idf rows.  No GPU."""
import os

import numpy as np
import pytest
import torch

import dssm_ref
from dssm_ref import DssmCase, PARAMS, sample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ['dssm_tiny', 'dssm_tiny_wide', 'dssm_drop_tiny']
ENTRY_POINTS = ('nnr_wbag_dims', 'nnr_wbag_fwd_ws_floats', 'nnr_wbag_fwd', 'nnr_wbag_bwd_ws_floats', 'nnr_wbag_bwd', 'nnr_cosine_loss',
                'nnr_tanh_drop_bwd')


@pytest.mark.parametrize('tag', CASES)
def test_the_restatement_reproduces_the_reference_fixture(tag):
    """float64 against the reference's fp32 logits, loss and gradients: 1e-5 of each tensor's max magnitude (dssm_drop_tiny: with the
    six recorded nn.Dropout masks, which pins the site order and the 1 / (1 - p) scale)."""
    case = DssmCase(tag)
    ui, uw, _, ni, nw, _ = case.batch()
    logits, loss, grads = dssm_ref.forward_backward(case.params(), ui, uw, ni, nw, case.masks(0), case.p)
    report = []

    def close(name, got, exp):
        got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
        err, mag = float(np.abs(got - exp).max()), float(np.abs(exp).max())
        report.append('%s %.2e (max %.2e)' % (name, err, mag))
        assert err <= 1e-5 * mag, (tag, name, err, mag)
    close('logits', logits.numpy(), case.expect('logits'))
    close('loss', loss.numpy(), case.expect('loss'))
    for k in PARAMS:
        close('d' + k, sample(grads[k].numpy()), case.expect('grad/' + k))
        assert abs(float(grads[k].norm()) - float(case.expect('gradnorm/' + k))) <= 1e-5 * max(float(case.expect('gradnorm/' + k)), 1e-30)
    print('%s: %s' % (tag, '; '.join(report)))
    assert float(case.expect('loss')) == float(case.expect('loss_step0'))
    if case.p > 0:
        rate = np.mean([float(m.float().mean()) for m in case.masks(0).values()])
        assert 0.3 < rate < 0.8                                                     # masks, not all-ones


def test_the_fixtures_have_the_stated_shape():
    t = DssmCase('dssm_tiny')
    assert (t.meta['batch_size'], t.meta['negative_sample_num'] + 1, t.meta['user_word_num'], t.meta['news_word_num'], t.meta['vocabulary_size'],
            t.meta['DSSM_hidden_dim'], t.meta['DSSM_feature_dim']) == (3, 3, 9, 4, 37, 6, 5)
    ui, uw, _, ni, nw, _ = t.batch()
    assert ui.shape == (3, 9) and ni.shape == (3, 3, 4) and ui.dtype == np.int64
    assert (uw == 0).any() and (nw == 0).any()                                      # zero-weight tails
    assert (nw != 0).any(axis=2).all() and (uw != 0).any(axis=1).all()             # no empty row
    assert np.intersect1d(ui[uw != 0], ni[nw != 0]).size > 0                         # ids shared by the two sides
    live = ni[nw != 0]
    assert np.unique(live).size < live.size                                          # ... and repeated across rows
    w = DssmCase('dssm_tiny_wide')
    assert (w.meta['DSSM_hidden_dim'], w.meta['DSSM_feature_dim'], w.meta['user_word_num']) == (512, 512, 70)
    d = DssmCase('dssm_drop_tiny')
    assert d.p == 0.5 and set(d.masks(0)) == set(dssm_ref.SITES) and d.masks(2)['news_bag'].shape == (3, 3, 4, 6)
    for tag in CASES:
        assert os.path.getsize(os.path.join(dssm_ref.GOLDEN, tag + '.npz')) < 400 * 1024
        s = DssmCase(tag).expect('eval/scores')
        o = 0
        for n in DssmCase(tag).expect('eval/sizes'):                                 # tiny-split scores without ties
            assert np.unique(s[o:o + n]).size == n
            o += n


@pytest.mark.parametrize('tag', CASES)
def test_state_dict_names_shapes_and_strict_load(tag):
    from nnr_amd.dssm import DSSM
    case = DssmCase(tag)
    model = DSSM(case.config())
    sd = model.state_dict()
    assert tuple(sd) == PARAMS
    assert {k: list(v.shape) for k, v in sd.items()} == case.meta['shapes']
    model.load_state_dict({k: torch.as_tensor(v) for k, v in case.params().items()}, strict=True)
    for k, v in case.params().items():
        assert np.array_equal(model.state_dict()[k].numpy(), v)


def test_initialize_follows_the_reference():
    from nnr_amd.dssm import DSSM
    torch.manual_seed(3)
    model = DSSM(DssmCase('dssm_tiny').config(vocabulary_size=400, DSSM_hidden_dim=48, DSSM_feature_dim=20))
    b3, b4 = model.W3.bias.detach().clone(), model.W4.bias.detach().clone()
    model.initialize()
    t = model.word_embedding.weight.detach()
    assert float(t.abs().max()) <= 0.1 and float(t.abs().max()) > 0.09 and abs(float(t.mean())) < 0.01
    gain = 5.0 / 3.0                                                                 # nn.init.calculate_gain('tanh')
    for w, (fo, fi) in ((model.W3.weight.detach(), (48, 48)), (model.W4.weight.detach(), (20, 48))):
        bound = gain * (6.0 / (fi + fo)) ** 0.5
        assert tuple(w.shape) == (fo, fi) and float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound
    assert torch.equal(model.W3.bias, b3) and torch.equal(model.W4.bias, b4)         # nn.Linear's default, untouched
    assert float(b3.abs().max()) <= 1.0 / 48 ** 0.5


def test_flags_and_defaults():
    from nnr_amd.dssm import make_dssm_config
    want = dict(mode='train', dev_model_path='best_model/DSSM/#1/DSSM', test_model_path='best_model/DSSM/#1/DSSM', device_id=0, seed=0,
                dataset='200k', news_word_num=200, user_word_num=3200, negative_sample_num=4, epoch=100, batch_size=64, lr=1e-4, weight_decay=0,
                gradient_clip_norm=4, dev_criterion='auc', early_stopping_epoch=5, word_embedding_dim=300, DSSM_hidden_dim=512,
                DSSM_feature_dim=512, dropout_rate=0)
    cwd = sorted(os.listdir('.'))
    cfg = make_dssm_config([])
    assert vars(cfg) == want
    assert sorted(os.listdir('.')) == cwd                                            # no side effects
    cfg = make_dssm_config(['--user_word_num', '64', '--DSSM_hidden_dim', '128', '--dropout_rate', '0.2', '--lr', '0.01'])
    assert (cfg.user_word_num, cfg.DSSM_hidden_dim, cfg.dropout_rate, cfg.lr) == (64, 128, 0.2, 0.01)
    with pytest.raises(SystemExit):
        make_dssm_config(['--dataset', 'huge'])


@pytest.mark.parametrize('over', [dict(DSSM_hidden_dim=1025), dict(user_word_num=4097), dict(user_word_num=0)], ids=str)
def test_constructor_refuses_sizes_beyond_the_kernels_rule(over, monkeypatch):
    from nnr_amd import _lib
    from nnr_amd.dssm import DSSM
    monkeypatch.setattr(_lib, 'lib', lambda: pytest.fail('the constructor must not call the library'))
    with pytest.raises(Exception, match='unsupported size'):
        DSSM(DssmCase('dssm_tiny').config(**over))
    DSSM(DssmCase('dssm_tiny').config(DSSM_hidden_dim=1024, user_word_num=4096, news_word_num=4096, vocabulary_size=3))


def test_the_restated_rule_is_the_librarys():
    from nnr_amd import _lib, ops
    L = _lib.lib()
    import ctypes as C
    chunk, ca, cb = C.c_int(), C.c_int(), C.c_int()
    for E, La, Lb in [(1, 1, 0), (1024, 4096, 4096), (1025, 1, 1), (0, 1, 1), (8, 4097, 1), (8, 0, 1), (8, 1, 4097), (8, 1, -1), (512, 3200, 200)]:
        rc = L.nnr_wbag_dims(E, La, Lb, C.addressof(chunk), C.addressof(ca), C.addressof(cb))
        assert (rc == 0) == ops.wbag_supported(E, La, Lb), (E, La, Lb, rc)
        assert rc in (0, _lib.NNR_ERR_UNSUPPORTED) and chunk.value > 0
        if rc == 0:
            assert ca.value == -(-La // chunk.value) and cb.value == -(-Lb // chunk.value)
            assert ops.wbag_dims(E, La, Lb) == (chunk.value, ca.value, cb.value)
    with pytest.raises(_lib.NnrHipError, match='unsupported size'):
        ops.wbag_dims(1025, 1, 1)
    ch = chunk.value
    assert L.nnr_wbag_fwd_ws_floats(64, 3200, 320, 200, 512) == (64 * -(-3200 // ch) + 320 * -(-200 // ch)) * 512
    assert L.nnr_wbag_bwd_ws_floats(0, 512) == 0 and L.nnr_wbag_bwd_ws_floats(1, 512) >= 2 * 512 and L.nnr_wbag_bwd_ws_floats(1, 1024) >= 2 * 1024


def test_plumbing():
    from nnr_amd import _lib
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES
        takes_stream = _lib.SIGNATURES[name].split()[-1] == 'stream'
        assert (L.nnr_tape_fn_id(name.encode()) >= 0) == takes_stream, name
    assert len(_lib.STRUCTS) == 6
    assert open(os.path.join(ROOT, 'nnr_amd', 'csrc', 'build.sh')).read().count(' dssm ') == 1
    src = open(os.path.join(ROOT, 'nnr_amd', 'csrc', 'dssm.hip')).read()
    assert 'atomicAdd(&g_cosine_arrived' in src and src.count('atomicAdd') == 1       # the arrival counter only: no float atomics


def test_cpu_tensors_are_refused():
    from nnr_amd import _lib
    from nnr_amd.dssm import DSSM, DssmCorpus, DssmTrainer
    case = DssmCase('dssm_tiny')
    model = DSSM(case.config())
    batch = [torch.as_tensor(v) for v in case.batch()]
    with pytest.raises(_lib.NnrHipError):
        model(*batch)
    with pytest.raises(_lib.NnrHipError):
        model.loss(*batch)
    corpus = DssmCorpus(case.expect('corpus/user_ids'), case.expect('corpus/user_w'), case.expect('corpus/news_ids'), case.expect('corpus/news_w'), 'cpu')
    assert corpus.vocabulary_size == int(max(case.expect('corpus/user_ids').max(), case.expect('corpus/news_ids').max())) + 1
    with pytest.raises(_lib.NnrHipError):
        model.forward_ids(corpus, torch.as_tensor(case.expect('in/user_sel')), torch.as_tensor(case.expect('in/news_sel')))
    with pytest.raises(_lib.NnrHipError):
        DssmTrainer(model, case.config()).train_step(batch)


def test_corpus_batches_are_ids_only():
    from nnr_amd.dssm import DssmCorpus
    case = DssmCase('dssm_tiny')
    beh = [(0, 1, [2, 3]), (1, 4, [0, 2, 3, 5, 6]), (2, 0, [1])]
    corpus = DssmCorpus(case.expect('corpus/user_ids'), case.expect('corpus/user_w'), case.expect('corpus/news_ids'), case.expect('corpus/news_w'), 'cpu',
                        behaviors=beh)
    rng = np.random.RandomState(0)
    neg = corpus.negative_sampling(4, rng.randint)
    assert tuple(neg.shape) == (3, 5) and neg.dtype == torch.int32
    assert neg[:, 0].tolist() == [1, 4, 0] and neg[0, 1:].tolist() == [2, 3, 2, 3] and neg[2, 1:].tolist() == [1, 1, 1, 1]
    assert sorted(set(neg[1, 1:].tolist())) == sorted(neg[1, 1:].tolist()) and set(neg[1, 1:].tolist()) <= {0, 2, 3, 5, 6}
    us, ns = corpus.train_batch(torch.tensor([2, 0]))
    assert us.tolist() == [2, 0] and ns.tolist() == [neg[2].tolist(), neg[0].tolist()] and us.dtype == ns.dtype == torch.int32
    ui, uw, ul, ni, nw, nl = corpus.gather(us, ns)
    assert ui.shape == (2, 9) and ni.shape == (2, 5, 4) and ui.dtype == torch.int64
    assert np.array_equal(uw.numpy(), case.expect('corpus/user_w')[[2, 0]]) and np.array_equal(ni[1, 2].numpy(), case.expect('corpus/news_ids')[neg[0, 2]])


def test_synthetic_tfidf_rows():
    from nnr_amd.synth import tfidf_rows
    ids, w = tfidf_rows(np.random.default_rng(5), 40, 64, 500)
    assert ids.shape == w.shape == (40, 64) and ids.dtype == np.int32 and w.dtype == np.float32
    live = w != 0
    n = live.sum(axis=1)
    assert (n == 0).sum() == 1 and n.max() <= 64 and np.unique(n).size > 5          # one fully empty row, tails of random length
    for r in range(40):
        assert live[r, :n[r]].all() and not live[r, n[r]:].any()                     # a prefix is live, the tail is zero
        assert (ids[r, n[r]:] == 0).all() and (ids[r, :n[r]] >= 1).all() and (ids[r, :n[r]] < 500).all()
        assert np.unique(ids[r, :n[r]]).size == n[r]                                 # distinct ids per row
        assert (np.diff(w[r, :n[r]]) <= 0).all() and (w[r, :n[r]] > 0).all()         # weights sorted descending
    counts = np.bincount(ids[live], minlength=500)
    assert counts[1:11].sum() > 5 * counts[250:260].sum()                            # Zipf: the head ids dominate
    a, b = tfidf_rows(np.random.default_rng(5), 40, 64, 500)
    assert np.array_equal(a, ids) and np.array_equal(b, w)
    one, _ = tfidf_rows(np.random.default_rng(1), 3, 8, 1)                            # a vocabulary of the padding id alone: nothing live
    assert not one.any()
