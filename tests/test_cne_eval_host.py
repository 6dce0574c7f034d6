"""De-duplicated evaluation of the rank-pairing CNE encoders, the parts that need no GPU (nnr_amd.evaluate.compute_scores_dedup /
dedup_refusal, the numpy restatement of nnr_cne_pair_triples in tests/cne_eval_ref.py, the entry point's declaration and refusals)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cne_eval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch_partners(tl, cl):
    """news_encoders.cne_history_dedup's own formula: order_c[rank_t], order_t[rank_c] from torch.sort(descending=True, stable=True)."""
    tl, cl = torch.from_numpy(np.asarray(tl, dtype=np.int64)), torch.from_numpy(np.asarray(cl, dtype=np.int64))
    order_t = torch.sort(tl, descending=True, stable=True)[1]
    order_c = torch.sort(cl, descending=True, stable=True)[1]
    rank_t, rank_c = torch.empty_like(order_t), torch.empty_like(order_c)
    ar = torch.arange(tl.numel())
    rank_t[order_t], rank_c[order_c] = ar, ar
    return order_c[rank_t].numpy(), order_t[rank_c].numpy()


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 350])
@pytest.mark.parametrize('kind', ['random', 'tied', 'distinct', 'extremes'])
def test_restatement_equals_the_encoders_formula(n, kind):
    rng = np.random.default_rng(100 * n + len(kind))
    if kind == 'random':
        tl, cl = rng.integers(1, 9, size=n), rng.integers(1, 17, size=n)
    elif kind == 'tied':
        tl, cl = np.full(n, 5), np.full(n, 11)
    elif kind == 'distinct':
        tl, cl = rng.permutation(n) + 1, rng.permutation(n) + 1
    else:
        tl, cl = rng.choice([1, 128], size=n), rng.choice([1, 128], size=n)
    pc, pt = R.call_partners(tl, cl)
    epc, ept = _torch_partners(tl, cl)
    np.testing.assert_array_equal(pc, epc)
    np.testing.assert_array_equal(pt, ept)
    if kind == 'tied':                                           # pure tie order: everybody is their own partner
        np.testing.assert_array_equal(pc, np.arange(n))
        np.testing.assert_array_equal(pt, np.arange(n))
    assert sorted(pc.tolist()) == list(range(n)) and sorted(pt.tolist()) == list(range(n))


def test_restatement_composes_the_reference_batches():
    """Two calls per batch of consecutive samples, the last batch short; the history call's sequence index is s * H + h; a window that starts
    at a batch boundary gives the rows of the whole split."""
    rng = np.random.default_rng(3)
    V, n, H, B = 30, 11, 4, 3
    tlen, clen = rng.integers(1, 6, size=V).astype(np.int32), rng.integers(1, 9, size=V).astype(np.int32)
    hist, cand = rng.integers(0, V, size=(n, H)).astype(np.int32), rng.integers(0, V, size=n).astype(np.int32)
    pc_h, pt_h, pc_c, pt_c = R.pair_triples(hist, cand, tlen, clen, B)
    for s in range(0, n, B):
        e = min(s + B, n)
        ids = hist[s:e].reshape(-1)
        pc, pt = _torch_partners(tlen[ids], clen[ids])
        np.testing.assert_array_equal(pc_h[s:e].reshape(-1), ids[pc])
        np.testing.assert_array_equal(pt_h[s:e].reshape(-1), ids[pt])
        pc, pt = _torch_partners(tlen[cand[s:e]], clen[cand[s:e]])
        np.testing.assert_array_equal(pc_c[s:e], cand[s:e][pc])
        np.testing.assert_array_equal(pt_c[s:e], cand[s:e][pt])
    part = R.pair_triples(hist, cand, tlen, clen, B, first=6, count=5)
    for whole, got in zip((pc_h, pt_h, pc_c, pt_c), part):
        np.testing.assert_array_equal(whole[6:], got)
    # one window over everything sees a repeated triple once; one window per batch counts it once per batch it occurs in
    assert R.distinct_triples(hist, cand, tlen, clen, B, 100) <= R.distinct_triples(hist, cand, tlen, clen, B, 1) <= n * (H + 1)
    np.testing.assert_array_equal(R.mask_lengths(np.array([[0, 0, 0], [1, 1, 0], [0, 1, 1]])), [1, 2, 3])


def _model(news, user, *extra):
    from nnr_amd.config import make_config
    from nnr_amd.model import Model
    return Model(make_config(['--news_encoder=' + news, '--user_encoder=' + user] + list(extra), corpus_sizes=dict(vocabulary_size=50, user_num=7)))


@pytest.mark.parametrize('news,user,extra,word', [('CNE', 'SUE', ['--tie_order=torch'], 'tie_order'), ('PNE', 'PUE', [], 'cne_gate'),
                                                  ('HDC', 'FIM', ['--click_predictor=FIM'], 'cne_gate'), ('CNN', 'ATT', [], 'cached'),
                                                  ('CNE_wo_CS', 'ATT', [], 'cached')])
def test_refusals_name_their_reason(news, user, extra, word):
    """Refused before the corpus is looked at (it is None here), with an NnrHipError that names the encoder and the reason."""
    from nnr_amd import evaluate as E, _lib
    m = _model(news, user, *extra)
    assert not E.dedup_supported(m) and word in E.dedup_refusal(m)
    with pytest.raises(_lib.NnrHipError, match=word) as e:
        E.compute_scores_dedup(m, None, 8)
    assert news in str(e.value)


def test_a_user_encoder_without_encode_user_is_refused():
    from nnr_amd import evaluate as E, _lib
    m = _model('CNE', 'ATT')
    assert E.dedup_supported(m) and E.dedup_refusal(m) is None

    class Plugin(torch.nn.Module):                               # a user encoder with the reference's forward() only
        pass
    m.user_encoder = Plugin()
    with pytest.raises(_lib.NnrHipError, match='encode_user') as e:
        E.compute_scores_dedup(m, None, 8)
    assert 'Plugin' in str(e.value)


@pytest.mark.parametrize('news,user', [('CNE', 'SUE'), ('CNE', 'ATT'), ('CNE_wo_CA', 'ATT')])
def test_supported_pairs(news, user):
    from nnr_amd import evaluate as E
    m = _model(news, user)
    assert E.dedup_supported(m) and not E.news_reps_cacheable(m) and not E.listwise_supported(m)


def test_keyword_plumbing(monkeypatch):
    """evaluate(dedup=True): a news_reps_cacheable model keeps today's path, a rank-pairing one takes the new form, the default is unchanged;
    run.fit hands its keyword on."""
    import inspect
    from nnr_amd import evaluate as E, run
    taken = []
    monkeypatch.setattr(E, 'compute_scores', lambda model, corpus, bs, cache='auto': taken.append('plain') or torch.zeros(3))
    monkeypatch.setattr(E, 'compute_scores_dedup', lambda model, corpus, bs, **kw: taken.append('dedup') or torch.zeros(3))
    monkeypatch.setattr(E, 'compute_scores_listwise', lambda model, corpus, sizes, bs, **kw: taken.append('listwise') or torch.zeros(3))
    monkeypatch.setattr(E, 'rank_metrics', lambda scores, labels, sizes: (torch.zeros(3, dtype=torch.int32), None, torch.zeros(4, dtype=torch.float64)))
    cached, paired = _model('CNN', 'ATT'), _model('CNE', 'SUE')
    for model, kw, want in ((cached, dict(dedup=True), 'plain'), (cached, dict(), 'plain'), (cached, dict(dedup=True, listwise=True), 'listwise'),
                            (paired, dict(), 'plain'), (paired, dict(listwise=True), 'plain'), (paired, dict(dedup=True), 'dedup'),
                            (paired, dict(dedup=True, listwise=True), 'dedup'), (_model('PNE', 'PUE'), dict(dedup=True), 'plain')):
        del taken[:]
        E.evaluate(model, None, [0, 1, 0], [3], 8, **kw)
        assert taken == [want], (type(model.news_encoder).__name__, kw, taken)
    assert inspect.signature(E.evaluate).parameters['dedup'].default is False
    assert inspect.signature(run.fit).parameters['dedup'].default is False
    assert 'dedup=dedup' in inspect.getsource(run.fit)


def test_entry_point_is_declared_listed_recordable_and_refuses_bad_arguments():
    from nnr_amd import _lib, evaluate, ops
    header = open(os.path.join(ROOT, 'include', 'nnr_hip.h')).read()
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert re.search(r'\bnnr_cne_pair_triples\s*\(', header)
    assert 'nnr_cne_pair_triples' in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), 'nnr_cne_pair_triples')
    L = _lib.lib()
    assert L.nnr_tape_fn_id(b'nnr_cne_pair_triples') >= 0
    assert callable(ops.cne_pair_triples) and callable(evaluate.compute_scores_dedup)
    # the refusals need no device: nothing is launched, no pointer is read (the non-null ones below point at host memory)
    buf = np.zeros(64, dtype=np.int32)
    p = buf.ctypes.data
    order = ('beh_history', 'cand', 'tlen', 'clen', 'n', 'H', 'n_news', 'batch_size', 'first', 'count', 'pc_hist', 'pt_hist', 'pc_cand', 'pt_cand', 'tmp')
    good = dict(beh_history=p, cand=p, tlen=p, clen=p, n=7, H=2, n_news=5, batch_size=3, first=3, count=4, pc_hist=p, pt_hist=p, pc_cand=p,
                pt_cand=p, tmp=p)
    bad = [{k: None} for k in order if good[k] == p] + [dict(H=0), dict(n_news=0), dict(batch_size=0), dict(count=0), dict(first=-3),
                                                         dict(first=2), dict(first=6, count=2), dict(count=5), dict(n=6), dict(count=2), dict(n=9)]
    for over in bad:
        a = dict(good, **over)
        assert L.nnr_cne_pair_triples(*[a[k] for k in order], None) == _lib.NNR_ERR_ARG, over
    assert (buf == 0).all()
    # the wrapper's own refusals come before any device work too
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32)
    for args in ((i32(4, 2), i32(3), i32(5), i32(5), 2), (i32(4, 2), i32(4), i32(5), i32(6), 2), (i32(4, 2).long(), i32(4), i32(5), i32(5), 2),
                 (i32(4, 2), i32(4), i32(5), i32(5), 0), (i32(4, 2), i32(4), i32(5), i32(5), 2, 1), (i32(4, 2), i32(4), i32(5), i32(5), 2, 2, 3), (i32(5, 2), i32(5), i32(5), i32(5), 2, 0, 3)):
        with pytest.raises(_lib.NnrHipError, match='cne_pair_triples'):
            ops.cne_pair_triples(*args)
