"""Listwise evaluation on the device (nnr_amd.evaluate.compute_scores_listwise, csrc/corpus.hip:list_scores_kernel).

Bars.  Op level: the float64 restatement of tests/list_eval_ref.py is the expectation; the kernel's bar is 4 x the error of the same formula
in fp32 on the CPU, never below 1e-6 x max |expected| (the bar of tests/test_hip_bow_gpu.py).  Model level, both from tests/test_hip_eval_gpu.py:
scores within 2e-5 of the reference's own util.compute_scores (tests/golden/eval_tiny_*.npz) and within 2e-6 of this package's
compute_scores(cache=True); ranks exact and means within 1e-12 where the reference's smallest in-impression score gap exceeds 1e-4 (that
leaves out DAE_GRU, an exact tie, and NAML_Title_ATT, 8.3e-5, and nothing else).  Every measured value is printed."""
import functools

import numpy as np
import pytest
import torch

import list_eval_ref
from golden_io import eval_fixture

pytestmark = pytest.mark.gpu

INDEPENDENT = ['tiny_MHSA_MHSA', 'tiny_CNN_ATT', 'tiny_DAE_ATT', 'tiny_DAE_GRU', 'tiny_Inception_ATT', 'tiny_NAML_Title_ATT',
               'tiny_CNN_SUE_wo_HCA', 'tiny_CNE_wo_CS_ATT']
AWARE = ['tiny_CNN_CATT', 'tiny_CNN_OMAP', 'tiny_CNN_SUE_wo_GCN', 'tiny_KCNN_CATT']
AMBIGUOUS = {'tiny_DAE_GRU', 'tiny_NAML_Title_ATT'}           # smallest in-impression gap of the reference's scores <= 1e-4


# ------------------------------------------------------------------------------------------------------------------ op level
def _run(ub, rb, row, cand, D, tail=7, runs=1):
    """The kernel on the first D columns of the buffers ub / rb (their row strides are the buffers' widths) -> `runs` score vectors, each
    with a NaN-filled guard tail behind its n entries."""
    from nnr_amd import ops
    u, r = torch.from_numpy(ub).cuda()[:, :D], torch.from_numpy(rb).cuda()[:, :D]
    rw, cd = torch.from_numpy(row).cuda(), torch.from_numpy(cand).cuda()
    outs = []
    for _ in range(runs):
        out = torch.full((len(row) + tail,), float('nan'), device='cuda')
        ops.list_scores(u, r, rw, cd, scores=out)
        outs.append(out.cpu().numpy())
    return outs


@pytest.mark.parametrize('n', [1, 5, 257])
@pytest.mark.parametrize('D', [1, 63, 64, 65, 400, 500])
def test_list_scores_against_float64(D, n):
    """Three user rows and three news rows, so that indices repeat; contiguous and padded row strides (ldu = D + 3 and ldr = D + 2 are no
    multiples of 4 at D = 400: the 4-byte path; D = 64, 400, 500 with ldu = ldr = D: the 16-byte path, D = 500 with a partial last chunk)."""
    for ldu in (D, D + 3):
        for ldr in (D, D + 2):
            ub, rb, row, cand = list_eval_ref.tables(3, 3, D, n, ldu, ldr, seed=1000 * D + n)
            exp = list_eval_ref.list_scores(ub[:, :D], rb[:, :D], row, cand)
            f32 = list_eval_ref.list_scores(ub[:, :D], rb[:, :D], row, cand, np.float32)
            e32, emax = float(np.abs(f32.astype(np.float64) - exp).max()), float(np.abs(exp).max())
            bar = max(4.0 * e32, 1e-6 * emax)
            a, b = _run(ub, rb, row, cand, D, runs=2)
            err = float(np.abs(a[:n].astype(np.float64) - exp).max())
            print('D %d n %d ldu %d ldr %d: fp32 formula %.3e, max|exp| %.3e, bar %.3e, kernel %.3e' % (D, n, ldu, ldr, e32, emax, bar, err))
            assert err <= bar, (D, n, ldu, ldr, err, bar)
            assert np.isnan(a[n:]).all() and len(a) == n + 7, 'entries beyond n were written'
            assert a[:n].tobytes() == b[:n].tobytes(), 'two runs differ'


def test_a_score_is_a_pure_function_of_its_two_rows():
    """One (row, cand) pair at the first and last sample, at neighbouring waves of one workgroup, at both ends of a grid trip (the grid is
    capped at 2048 workgroups of four samples) -- among random other pairs -- in a 16-byte-path launch, in two 4-byte-path launches (ldr no
    multiple of 4; a user table that starts 4 bytes off a 16-byte boundary) and in a launch of five samples: the same bits everywhere, and
    every launch equals every other bit for bit."""
    from nnr_amd import ops
    D, n = 400, 2 * 8192 + 5
    ub, rb, row, cand = list_eval_ref.tables(3, 3, D, n, D, D, seed=7)
    spots = [0, 1, 2, 3, 4, 255, 256, 8191, 8192, 8193, n - 1]
    row[spots], cand[spots] = 1, 2
    vec, = _run(ub, rb, row, cand, D)
    rb2 = np.full((3, D + 2), np.nan, dtype=np.float32)
    rb2[:, :D] = rb
    sca, = _run(ub, rb2, row, cand, D)
    flat = torch.full((3 * D + 1,), float('nan'), device='cuda')
    flat[1:] = torch.from_numpy(ub).cuda().reshape(-1)
    off = flat[1:].view(3, D)
    assert off.data_ptr() % 16 == 4
    mis = ops.list_scores(off, torch.from_numpy(rb).cuda(), torch.from_numpy(row).cuda(), torch.from_numpy(cand).cuda()).cpu().numpy()
    small, = _run(ub, rb, row[:5].copy(), cand[:5].copy(), D)
    assert vec[:n].tobytes() == sca[:n].tobytes() == mis.tobytes(), 'the load paths disagree'
    assert small[:5].tobytes() == vec[:5].tobytes(), 'the grid matters'
    pair = row.astype(np.int64) * 3 + cand
    for p in range(9):
        vals = vec[:n][pair == p]
        assert vals.size and (vals.view(np.uint32) == vals.view(np.uint32)[0]).all(), 'pair %d: a score depends on where the sample stands' % p
    assert len(set(vec[spots].view(np.uint32).tolist())) == 1


def test_wrapper_refuses_indices_outside_the_tables():
    """The kernel trusts its indices; the wrapper reads their ranges back and raises before the launch: the score buffer stays as it was."""
    from nnr_amd import ops, _lib
    u, r = torch.randn(3, 8, device='cuda'), torch.randn(4, 8, device='cuda')
    good = torch.tensor([0, 1, 2, 0], dtype=torch.int32, device='cuda')
    for row, cand in ((torch.tensor([0, 3, 1, 0]), good), (torch.tensor([0, -1, 1, 0]), good), (good, torch.tensor([0, 4, 1, 0])),
                      (good, torch.tensor([-2, 0, 1, 0]))):
        out = torch.full((4,), float('nan'), device='cuda')
        with pytest.raises(_lib.NnrHipError, match='indices'):
            ops.list_scores(u, r, row.to(device='cuda', dtype=torch.int32), cand.to(device='cuda', dtype=torch.int32), scores=out)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())
    assert bool(torch.isfinite(ops.list_scores(u, r, good, good)).all())


# ------------------------------------------------------------------------------------------------------------------ the reference's scores
@functools.lru_cache(maxsize=None)
def _fixture(tag):
    """(z, model in train mode on the GPU, dev corpus, compute_scores(cache=True) as numpy): built once per fixture, then only read."""
    from nnr_amd import evaluate as E
    z, model = eval_fixture(tag)
    model = model.cuda().train()
    dc = E.dev_corpus({k: z[k] for k in z.files}, 'cuda', int(z['category_num']))
    cached = E.compute_scores(model, dc, batch_size=8, cache=True)
    assert E.LAST_STATS['mode'] == 'cached' and model.training
    return z, model, dc, cached.cpu().numpy()


def _min_gap(z):
    gaps, o = [], 0
    for n in z['sizes']:
        s = np.sort(z['scores'][o:o + n])
        gaps.append(np.diff(s).min() if n > 1 else 1.0)
        o += n
    return float(min(gaps))


def _check_against_reference(tag, stats_rows, **kw):
    from nnr_amd import evaluate as E
    z, model, dc, cached = _fixture(tag)
    assert E.listwise_supported(model) and model.user_encoder.candidate_independent == (tag in INDEPENDENT)
    for k in ('beh_user', 'beh_history', 'beh_history_mask'):               # the fixture is a list split: rows equal inside each impression
        o = 0
        for n in z['sizes']:
            assert (z[k][o:o + n] == z[k][o]).all()
            o += n
    scores = E.compute_scores_listwise(model, dc, z['sizes'], batch_size=8, **kw)
    st = dict(E.LAST_STATS)
    assert model.training, 'the model must come back in train mode'
    got = scores.cpu().numpy()
    assert scores.dtype == torch.float32 and got.shape == z['scores'].shape
    e_ref, e_own = float(np.abs(got - z['scores']).max()), float(np.abs(got - cached).max())
    print('%s %s: |listwise - reference| %.3e, |listwise - cached| %.3e, user rows %d for %d samples' % (tag, kw, e_ref, e_own, st['user_rows'], len(got)))
    assert e_ref <= 2e-5 and e_own <= 2e-6, (e_ref, e_own)
    assert st['mode'] == 'listwise' and st['per_sample_user_rows'] == len(got) and st['encoder_rows'] >= 1
    assert stats_rows(st['user_rows'], z['sizes']), st
    ranks, per, mean = E.rank_metrics(scores, torch.from_numpy(z['labels']), z['sizes'])
    gap = _min_gap(z)
    assert gap > 1e-4 or tag in AMBIGUOUS, (tag, gap)                       # nothing else is left out
    if gap > 1e-4:
        np.testing.assert_array_equal(ranks.cpu().numpy(), z['ranks'])
        np.testing.assert_allclose(mean.cpu().numpy(), z['metrics'], rtol=0, atol=1e-12)
        means, ranks2 = E.evaluate(model, dc, z['labels'], z['sizes'], 8, listwise=True)
        assert E.LAST_STATS['mode'] == 'listwise' and model.training
        np.testing.assert_allclose(np.asarray(means), z['metrics'], rtol=0, atol=1e-12)
        np.testing.assert_array_equal(ranks2.cpu().numpy(), z['ranks'])
    return st


@pytest.mark.parametrize('dedup', [True, False])
@pytest.mark.parametrize('tag', INDEPENDENT)
def test_independent_encoders_give_the_reference_scores(tag, dedup):
    st = _check_against_reference(tag, lambda rows, sizes: rows == len(sizes) if not dedup else 1 <= rows <= len(sizes), dedup_users=dedup)
    assert st['candidates_per_row'] is None


@pytest.mark.parametrize('K', [1, 3, 8])
@pytest.mark.parametrize('tag', AWARE)
def test_candidate_aware_encoders_give_the_reference_scores(tag, K):
    """K = 3 pads the second rows of the two impressions of size 4; K = 8 pads every row."""
    st = _check_against_reference(tag, lambda rows, sizes: rows == sum(-(-int(s) // K) for s in sizes), candidates_per_row=K)
    assert st['candidates_per_row'] == K


def test_evaluate_without_the_keyword_and_for_unsupported_models_keeps_its_path():
    from nnr_amd import evaluate as E
    z, model, dc, _ = _fixture('tiny_CNN_ATT')
    means, _ = E.evaluate(model, dc, z['labels'], z['sizes'], 8)
    assert E.LAST_STATS['mode'] == 'cached'
    np.testing.assert_allclose(np.asarray(means), z['metrics'], rtol=0, atol=1e-12)
    z, model = eval_fixture('tiny_CNE_SUE_stable')
    model = model.cuda().train()
    dc = E.dev_corpus({k: z[k] for k in z.files}, 'cuda', int(z['category_num']))
    assert not E.listwise_supported(model)
    means, _ = E.evaluate(model, dc, z['labels'], z['sizes'], 8, listwise=True)
    assert E.LAST_STATS['mode'] == 'per-sample' and model.training
    with pytest.raises(Exception, match='batch_independent') as e:
        E.compute_scores_listwise(model, dc, z['sizes'], 8)
    assert 'CNE' in str(e.value) and model.training


def test_refusals_of_a_split_that_is_no_list_split():
    from nnr_amd import evaluate as E
    z, model, dc, _ = _fixture('tiny_CNN_CATT')
    arrays = {k: z[k].copy() for k in z.files}
    j = int(z['sizes'][0]) + 1                                               # second sample of the second impression
    arrays['beh_history'][j, 0] = arrays['beh_history'][j, 0] % 50 + 1
    assert (arrays['beh_history'][j] != z['beh_history'][j]).any()
    bad = E.dev_corpus(arrays, 'cuda', int(z['category_num']))
    E.LAST_STATS.clear()
    with pytest.raises(ValueError, match='differs from its impression'):
        E.compute_scores_listwise(model, bad, z['sizes'], 8)
    assert not E.LAST_STATS and model.training
    arrays = {k: z[k].copy() for k in z.files}
    arrays['beh_user'][j] += 1
    with pytest.raises(ValueError, match='differs from its impression'):
        E.compute_scores_listwise(model, E.dev_corpus(arrays, 'cuda', int(z['category_num'])), z['sizes'], 8)
    for sizes in ([3, 4, 6, 4], [3, 4, 6, 4, 4]):
        with pytest.raises(ValueError, match='sizes sum to'):
            E.compute_scores_listwise(model, dc, sizes, 8)
    with pytest.raises(ValueError):
        E.compute_scores_listwise(model, dc, [3, 4, 6, 4, 3, 0], 8)


# ------------------------------------------------------------------------------------------------------------------ neighbours do not matter
def _synth_model(args, vocab, seed=0):
    from nnr_amd.config import make_config
    from nnr_amd.model import Model
    cfg = make_config(args, corpus_sizes=dict(vocabulary_size=vocab))
    torch.manual_seed(seed)
    model = Model(cfg)
    model.initialize()
    return model.cuda()


def _tiny_config(news, user):
    """The configuration of the tiny fixtures (tests/golden/eval_tiny_CNN_CATT.npz) with another encoder pair."""
    import os
    from types import SimpleNamespace
    from golden_io import GOLDEN_DIR
    z = np.load(os.path.join(GOLDEN_DIR, 'eval_tiny_CNN_CATT.npz'))
    cast = {'int': int, 'float': float, 'str': str, 'bool': lambda v: v == 'True'}
    cfg = SimpleNamespace(**{k: cast[t](v) for k, v, t in zip(z['cfg_keys'], z['cfg_vals'], z['cfg_types'])})
    cfg.news_encoder, cfg.user_encoder, cfg.tie_order = news, user, str(z['tie_order'])
    return cfg


@pytest.mark.parametrize('news,user', [('MHSA', 'SUE'), ('CNN', 'CATT')])
def test_row_mates_do_not_change_a_candidates_score(news, user):
    """No cacheable fixture holds SUE: models from Model.initialize() under a fixed seed, a synthetic split of 24 impressions of 1..20
    candidates.  A candidate scored in a row of 8 (with its row-mates, pad slots included) = scored alone = the cached per-sample form, within
    the 2e-6 of test_hip_eval_gpu.py.  That bar is an absolute one, set on the tiny fixtures whose scores are below 1; the models here have
    the tiny fixtures' widths so that it means the same thing (about 16 ulp of 1.0).  At the default widths an initialised MHSA+SUE scores
    up to 1.3e2, where one ulp is 1.5e-5 and an absolute 2e-6 would ask for bit equality of two GEMM shapes: measured there, K = 8 against
    K = 1 and against the cached form both 4.6e-5 = 3 ulp (the MIND-shaped test below holds that regime to its relative bar)."""
    from nnr_amd import evaluate as E
    from nnr_amd.corpus import from_synth_lists
    from nnr_amd.model import Model
    from nnr_amd.synth import SynthSpec, SynthCorpus
    cfg = _tiny_config(news, user)
    torch.manual_seed(0)
    model = Model(cfg)
    model.initialize()
    model = model.cuda().train()
    synth = SynthCorpus(SynthSpec(vocabulary_size=cfg.vocabulary_size, category_num=cfg.category_num, subCategory_num=cfg.subCategory_num,
                                  max_title_length=cfg.max_title_length, max_abstract_length=cfg.max_abstract_length,
                                  max_history_num=cfg.max_history_num, negative_sample_num=cfg.negative_sample_num, news_pool=150,
                                  title_len_mean=5.0, content_len_mean=9.0, seed=5))
    rng = np.random.default_rng(11)
    sizes = rng.integers(1, 21, size=24)
    dc = from_synth_lists(synth, sizes, rng, 'cuda')
    k8 = E.compute_scores_listwise(model, dc, sizes, 16, candidates_per_row=8)
    assert E.LAST_STATS['user_rows'] == int(sum(-(-int(s) // 8) for s in sizes))
    k1 = E.compute_scores_listwise(model, dc, sizes, 16, candidates_per_row=1)
    assert E.LAST_STATS['user_rows'] == int(sizes.sum())
    cached = E.compute_scores(model, dc, 16, cache=True)
    a, b = float((k8 - k1).abs().max()), float((k8 - cached).abs().max())
    top, spread = float(cached.abs().max()), float(cached.std())
    print('%s+%s: |K8 - K1| %.3e, |K8 - cached| %.3e, max |score| %.3e, std %.3e' % (news, user, a, b, top, spread))
    assert top > 1e-3 and spread > 1e-4, 'degenerate scores would pass any bar'
    assert a <= 2e-6 and b <= 2e-6, (a, b)


@pytest.mark.parametrize('user', ['ATT', 'MHSA', 'GRU', 'PUE', 'SUE_wo_HCA'])
def test_flagged_encoders_never_read_the_candidates(user):
    from nnr_amd import user_encoders as U
    from nnr_amd.config import make_config
    from nnr_amd.corpus import history_graph
    from nnr_amd.model import Model
    assert getattr(U, user).candidate_independent
    cfg = make_config(['--news_encoder=' + ('PNE' if user == 'PUE' else 'CNN'), '--user_encoder=' + user, '--max_history_num=10'],
                      corpus_sizes=dict(vocabulary_size=60, user_num=9))
    torch.manual_seed(3)
    model = Model(cfg)
    model.initialize()
    model = model.cuda().eval()
    ue = model.user_encoder
    B, H, D = 5, 10, ue.news_embedding_dim
    g = torch.Generator().manual_seed(4)
    hist = torch.randn(B, H, D, generator=g).cuda()
    counts = torch.tensor([0, 1, 4, 10, 7])
    mask = (torch.arange(H)[None, :] < counts[:, None]).cuda()
    extra = (model.user_rows(torch.tensor([0, 3, 3, 8, 1]).cuda()),) if ue.needs_user_embedding else ()
    cats = torch.randint(0, cfg.category_num, (B, H), generator=g).to(torch.int32).cuda()
    outs = []
    with torch.no_grad():
        for c in (torch.zeros(B, 1, D).cuda(), 3.0 * torch.randn(B, 1, D, generator=g).cuda()):
            graph = cmask = cidx = None
            if getattr(ue, 'needs_history_graph', False):
                graph, cmask, cidx = history_graph(cats, mask, cfg.category_num)
            outs.append(ue.encode_user(hist, mask, graph, cmask, cidx, c, *extra))
    assert tuple(outs[0].shape) == (B, 1, D) and torch.equal(outs[0], outs[1])
    assert float(outs[0].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------ MIND-shaped
@functools.lru_cache(maxsize=None)
def _mind_split():
    from nnr_amd.corpus import from_synth_lists
    from nnr_amd.synth import SynthSpec, SynthCorpus
    synth = SynthCorpus(SynthSpec(vocabulary_size=5000, news_pool=20000, seed=2))
    rng = np.random.default_rng(1)
    sizes = rng.integers(1, 61, size=600)
    return from_synth_lists(synth, sizes, rng, 'cuda'), sizes


@pytest.mark.parametrize('user', ['MHSA', 'SUE'])
def test_listwise_evaluation_on_a_mind_shaped_split(user):
    """600 behaviours over a 20 000-news pool with up to 50-news histories, lists of 1..60 candidates: the scores of the cached per-sample
    form (the bar of test_hip_eval_gpu's MIND-shaped test) with the user encoder run once per impression / once per 8 candidates."""
    from nnr_amd import evaluate as E
    dc, sizes = _mind_split()
    model = _synth_model(['--news_encoder=MHSA', '--user_encoder=' + user], 5000)
    a = E.compute_scores_listwise(model, dc, sizes, 256)
    st = dict(E.LAST_STATS)
    b = E.compute_scores(model, dc, 256, cache=True)
    err, top = float((a - b).abs().max()), float(b.abs().max())
    print('MHSA+%s: %d samples, %d user rows, |listwise - cached| %.3e, max |score| %.3e' % (user, dc.num, st['user_rows'], err, top))
    assert err <= 1e-5 * max(1.0, top)
    assert st['per_sample_user_rows'] == dc.num == int(sizes.sum())
    if user == 'MHSA':
        assert 1 <= st['user_rows'] <= len(sizes) and st['candidates_per_row'] is None
    else:
        assert st['user_rows'] == int(sum(-(-int(s) // 8) for s in sizes)) and st['candidates_per_row'] == 8
