"""The archive form of recommend / rank_in_pool without a device: the float64 restatement tests/archive_rank_ref.py
against recommend_ref at its three exact corners, the header's operation sequence in float32 against the band, the two entry points'
declaration, listing, export, tape registration and argument refusals, the pool_archives flag, and recommend_refusal."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import archive_rank_ref as AR
import pool_rank_ref as P
import recommend_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ints(seed, *shape):
    return np.random.default_rng(seed).integers(-2, 3, size=shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_one_archive_is_recommend_ref():
    user, reps = _ints(1, 7, 1, 5), _ints(2, 40, 5)
    rng = np.random.default_rng(3)
    nu, nr = rng.standard_normal((7, 1, 5)), rng.standard_normal((40, 5))
    for u3, r, scale in ((user, reps, 0.0), (user, reps, 0.7), (nu, nr, 0.0), (nu, nr, -1.3)):
        np.testing.assert_array_equal(AR.scores64(u3, r, scale), R.scores64(u3[:, 0], r))
        np.testing.assert_array_equal(AR.scores32(u3, r, scale).view(np.uint32), R.fma_chain32(u3[:, 0], r).view(np.uint32))
    el = AR.eligible(7, 40, None, rng.integers(-1, 42, size=(7, 4)))
    s = AR.scores64(user, reps, 0.4)
    for K in (1, 5, 64):
        for got, want in zip(AR.topk(s, el, K), R.topk(R.scores64(user[:, 0], reps), el, K)):
            np.testing.assert_array_equal(got, want)
    t_off, t_news = np.array([0, 2, 2, 3, 3, 3, 6, 7]), np.array([0, 39, 5, 1, 1, 38, 7])
    for got, want in zip(AR.ranks(s, el, t_off, t_news), P.ranks(R.scores64(user[:, 0], reps), el, t_off, t_news)):
        np.testing.assert_array_equal(got, want)
    # with one archive the first term of the band is recommend_ref's bound, and the brackets built on it contain recommend_ref's
    np.testing.assert_array_less(R.bound(nu[:, 0], nr), AR.band(nu, nr, 0.5) + 1e-300)
    lo, hi = AR.bracket(AR.scores64(nu, nr, 0.5), R.bound(nu[:, 0], nr), AR.eligible(7, 40), t_off, t_news)
    plo, phi = P.bracket(nu[:, 0], nr, AR.eligible(7, 40), t_off, t_news)
    np.testing.assert_array_equal(lo, plo)
    np.testing.assert_array_equal(hi, phi)


@pytest.mark.parametrize('A', [2, 3, 4, 16])
def test_scale_zero_is_the_mean(A):
    user, reps = _ints(10 + A, 6, A, 9), _ints(20 + A, 50, 9)
    mean = sum(R.scores64(user[:, a], reps) for a in range(A)) / A            # small integers: exact in any order
    np.testing.assert_array_equal(AR.scores64(user, reps, 0.0), mean)
    np.testing.assert_array_equal(AR.scores32(user, reps, 0.0), mean.astype(np.float32))
    rng = np.random.default_rng(A)
    nu, nr = rng.standard_normal((6, A, 33)).astype(np.float32), rng.standard_normal((50, 33)).astype(np.float32)
    acc = R.fma_chain32(nu[:, 0], nr)                                          # the header: (s_0 + .. + s_{A-1}) / A summed in ascending a, in fp32
    for a in range(1, A):
        acc = (acc + R.fma_chain32(nu[:, a], nr)).astype(np.float32)
    np.testing.assert_array_equal(AR.scores32(nu, nr, 0.0).view(np.uint32), (acc / np.float32(A)).astype(np.float32).view(np.uint32))


@pytest.mark.parametrize('A', [2, 4])
def test_equal_archives_give_the_single_row(A):
    rng = np.random.default_rng(30 + A)
    one, reps = rng.standard_normal((5, 1, 37)).astype(np.float32), rng.standard_normal((64, 37)).astype(np.float32)
    user = np.repeat(one, A, axis=1)
    for scale in (0.0, 0.16, -2.0):
        np.testing.assert_allclose(AR.scores64(user, reps, scale), R.scores64(one[:, 0], reps), rtol=1e-15, atol=0)
        np.testing.assert_array_equal(AR.scores32(user, reps, scale).view(np.uint32), R.fma_chain32(one[:, 0], reps).view(np.uint32))


@pytest.mark.parametrize('A,D,mult', [(2, 30, 1.0), (3, 100, 1.0), (16, 100, 1.0), (16, 500, 1.0), (16, 100, 8.0), (5, 64, -8.0)])
def test_the_stated_sequence_stays_inside_the_band(A, D, mult):
    """The header's sequence in float32 (combine32 over the fmaf chains) against float64: inside B everywhere, and by a wide margin."""
    rng = np.random.default_rng(A * 1000 + D)
    user, reps = rng.standard_normal((12, A, D)).astype(np.float32), rng.standard_normal((200, D)).astype(np.float32)
    scale = mult / np.sqrt(D)
    ratio = np.abs(AR.scores32(user, reps, scale).astype(np.float64) - AR.scores64(user, reps, scale)) / AR.band(user, reps, scale)
    print('A %d D %d scale %.4f: worst |fp32 sequence - float64| / B = %.4f' % (A, D, scale, ratio.max()))
    assert ratio.max() < 0.1


def test_combine32_is_the_softmax_weighted_sum_in_any_arrival_order():
    """Ascending, descending and mixed s_a (every branch of the running extreme), both signs of scale, against float64."""
    rng = np.random.default_rng(5)
    s = rng.standard_normal((300, 7)).astype(np.float32) * 4
    for arr in (np.sort(s, axis=1), -np.sort(-s, axis=1), s):
        for scale in (0.0, 0.3, 2.0, -0.8):
            want = AR.combine64(arr.astype(np.float64)[:, :, None], scale)[:, 0]
            np.testing.assert_allclose(AR.combine32(arr, scale), want, rtol=2e-6, atol=2e-6)


# ------------------------------------------------------------------------------------------------------------------ the entry points
TOPK_ORDER = ('user', 'n_user', 'ldu', 'A', 'lda', 'scale', 'reps', 'n_reps', 'ldr', 'D', 'valid', 'exclude', 'E', 'ld_ex', 'K', 'idx', 'score',
              'workspace', 'workspace_bytes')
RANK_ORDER = ('user', 'n_user', 'ldu', 'A', 'lda', 'scale', 'reps', 'n_reps', 'ldr', 'D', 'valid', 'exclude', 'E', 'ld_ex', 't_off', 't_news',
              'n_target', 'ahead', 't_score', 'pool_size', 'workspace', 'workspace_bytes')


def test_entry_points_are_declared_listed_recordable_and_refuse_bad_arguments():
    from nnr_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'nnr_hip.h')).read()
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for name, order in (('nnr_topk_archive_scores', TOPK_ORDER), ('nnr_pool_archive_ranks', RANK_ORDER)):
        m = re.search(r'\bint\s+%s\s*\(([^;]*)\);' % name, header)
        assert m, name
        params = [p.split()[-1].lstrip('*') for p in m.group(1).split(',')]
        assert tuple(params[:-1]) == order and params[-1] == 'stream', (name, params)
        assert name in _lib.SIGNATURES and len(_lib.kinds(name)) == len(order) + 1 and hasattr(raw, name)
        assert L.nnr_tape_fn_id(name.encode()) >= 0 and L.nnr_tape_fn_nargs(L.nnr_tape_fn_id(name.encode())) == len(order)
    for word in ('combine', 'fma(den, e, 1)', 'num / den', 'scale = 0', 'A = 1'):
        assert word in header, word
    # the refusals need no device: nothing is launched, no pointer is read (the non-null ones below point at host memory)
    buf = np.zeros(256, dtype=np.float32)
    p = buf.ctypes.data
    common = dict(user=p, n_user=3, ldu=12, A=3, lda=4, scale=0.5, reps=p, n_reps=300, ldr=4, D=4, valid=None, exclude=None, E=0, ld_ex=0,
                  workspace=None, workspace_bytes=0)
    assert _lib.lib().nnr_topk_workspace_bytes(3, 300, 5) == 0 and _lib.lib().nnr_pool_rank_workspace_bytes(3, 300, 2) == 0
    bad = [dict(A=0), dict(A=-1), dict(lda=3), dict(lda=0), dict(ldu=11), dict(ldu=4), dict(scale=float('nan')), dict(scale=float('inf')),
           dict(scale=float('-inf')), dict(user=None), dict(reps=None), dict(n_user=0), dict(n_reps=0), dict(D=0), dict(ldr=3), dict(E=-1),
           dict(E=2, ld_ex=2), dict(E=2, ld_ex=1, exclude=p), dict(A=17, ldu=68, lda=3)]
    topk = dict(common, K=5, idx=p, score=p)
    rank = dict(common, t_off=p, t_news=p, n_target=2, ahead=p, t_score=p, pool_size=p)
    for over in bad + [dict(K=0), dict(idx=None), dict(score=None), dict(A=17, ldu=68, K=0)]:
        a = dict(topk, **over)
        assert L.nnr_topk_archive_scores(*[a[k] for k in TOPK_ORDER], None) == _lib.NNR_ERR_ARG, over
    for over in bad + [dict(n_target=-1), dict(t_off=None), dict(pool_size=None), dict(t_news=None), dict(ahead=None), dict(t_score=None)]:
        a = dict(rank, **over)
        assert L.nnr_pool_archive_ranks(*[a[k] for k in RANK_ORDER], None) == _lib.NNR_ERR_ARG, over
    for over in (dict(A=17, ldu=68), dict(A=1000, ldu=4000), dict(K=65)):
        a = dict(topk, **over)
        assert L.nnr_topk_archive_scores(*[a[k] for k in TOPK_ORDER], None) == _lib.NNR_ERR_UNSUPPORTED, over
    for over in (dict(A=17, ldu=68), dict(n_target=2 ** 31)):
        a = dict(rank, **over)
        assert L.nnr_pool_archive_ranks(*[a[k] for k in RANK_ORDER], None) == _lib.NNR_ERR_UNSUPPORTED, over
    assert (buf == 0).all()


def test_ops_refuse_a_malformed_archive_table_before_any_launch():
    import torch
    from nnr_amd import _lib, ops
    reps = torch.zeros(9, 4)
    for user, kw in ((torch.zeros(3, 12), dict(archives=0)), (torch.zeros(3, 12), dict(archives=True)), (torch.zeros(3, 11), dict(archives=3)),
                     (torch.zeros(3, 12), dict(archives=3, lda=3)), (torch.zeros(3, 12), dict(archives=3, lda=5)),
                     (torch.zeros(3, 2, 4), dict(archives=3)), (torch.zeros(3, 3, 5), dict(archives=3)),
                     (torch.zeros(3, 1, 4).expand(3, 3, 4), dict(archives=3)), (torch.zeros(3, 12), dict(archives=3, scale=float('nan')))):
        with pytest.raises(_lib.NnrHipError, match='archives|scale'):
            ops.topk_scores(user, reps, 2, **kw)
        with pytest.raises(_lib.NnrHipError, match='archives|scale'):
            ops.pool_ranks(user, reps, torch.zeros(4, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), **kw)
    assert [p.default for n, p in inspect.signature(ops.topk_scores).parameters.items() if n in ('archives', 'lda', 'scale')] == [1, None, 0.0]
    assert [p.default for n, p in inspect.signature(ops.pool_ranks).parameters.items() if n in ('archives', 'lda', 'scale')] == [1, None, 0.0]


# ------------------------------------------------------------------------------------------------------------------ the flag and the refusal
def _model(news, user):
    from nnr_amd.config import make_config
    from nnr_amd.model import Model
    return Model(make_config(['--news_encoder=' + news, '--user_encoder=' + user], corpus_sizes=dict(vocabulary_size=50, user_num=7)))


def test_pool_archives_is_declared_on_the_base_and_true_for_omap_alone():
    from nnr_amd import user_encoders as U
    assert 'pool_archives' in vars(U.UserEncoder) and vars(U.UserEncoder)['pool_archives'] is False
    users = {n: c for n, c in inspect.getmembers(U, inspect.isclass) if issubclass(c, U.UserEncoder) and c is not U.UserEncoder
             and not n.startswith('_')}
    assert all(type(c.pool_archives) is bool for c in users.values())
    assert {n for n, c in users.items() if c.pool_archives} == {'OMAP'}
    assert U.OMAP.candidate_independent is False and callable(U.OMAP.encode_archives)
    for src in ('evaluate.py', 'model.py'):
        text = open(os.path.join(ROOT, 'nnr_amd', src)).read()
        assert not re.search(r'getattr\([^)]*pool_archives', text), src
    omap = _model('CNN', 'OMAP').user_encoder
    assert omap.archive_scale == 1.0 / np.sqrt(float(omap.news_embedding_dim)) and omap.OMAP_head_num <= 16


def test_recommend_refusal_admits_omap_and_no_other_candidate_aware_encoder():
    from nnr_amd import evaluate as E
    """The archive form is asked for: recommend_refusal(model, archives=True).  Without the keyword every answer is the one recommend gave before
    (tests/test_recommend_host.py pins CNN+OMAP among them), with a hint at the keyword for OMAP."""
    for news in ('CNN', 'MHSA'):
        assert E.recommend_refusal(_model(news, 'OMAP'), archives=True) is None
        assert E.recommend_refusal(_model(news, 'ATT'), archives=True) is None and E.recommend_refusal(_model(news, 'ATT')) is None
        why = E.recommend_refusal(_model(news, 'OMAP'))
        assert why and all(w in why for w in ('candidate_independent', 'OMAP', 'archives=True')), why
    for archives in (False, True):
        for news, user, word in (('CNN', 'CATT', 'candidate_independent'), ('MHSA', 'SUE', 'candidate_independent'),
                                 ('CNN', 'SUE_wo_GCN', 'candidate_independent'), ('CNE', 'OMAP', 'batch_independent')):
            why = E.recommend_refusal(_model(news, user), archives=archives)
            assert why is not None and word in why, (news, user, why)
            if user != 'OMAP':
                assert 'pass archives=True' not in why
        assert 'CATT' in E.recommend_refusal(_model('CNN', 'CATT'), archives) and 'pool_archives' in E.recommend_refusal(_model('CNN', 'CATT'), archives)
    assert [inspect.signature(f).parameters['archives'].default for f in (E.recommend_refusal, E.recommend, E.rank_in_pool)] == [False] * 3
