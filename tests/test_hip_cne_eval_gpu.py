"""De-duplicated evaluation of the rank-pairing CNE encoders on the device (nnr_amd.evaluate.compute_scores_dedup,
csrc/corpus.hip:cne_pair_triples_kernel).

Bars.  The plan kernel does integer work only: its output equals the numpy restatement (tests/cne_eval_ref.py) and its own second run bit
for bit.  End to end the new form regroups the rows of the encoder's products and changes nothing else, so its bar against the per-sample form
is the one tests/test_hip_list_eval_gpu.py holds listwise against cached scores to, 2e-6 absolute (BAR; the models here have tiny widths, so
scores are of order 1 at most and the bar means about 16 ulp of 1.0, as there); ranks and the four means are compared exactly, which means
something because every impression's smallest score gap in the per-sample form is asserted to exceed 100 x BAR.  Every measured value is
printed."""
import functools

import numpy as np
import pytest
import torch

import cne_eval_ref as R

pytestmark = pytest.mark.gpu

BAR = 2e-6                                                       # tests/test_hip_list_eval_gpu.py: |listwise - cached| <= 2e-6


# ------------------------------------------------------------------------------------------------------------------ the plan kernel
def _lengths(kind, V, rng):
    if kind == 'random':
        return rng.integers(1, 9, size=V), rng.integers(1, 17, size=V)
    if kind == 'tied':
        return np.full(V, 7), np.full(V, 12)
    if kind == 'distinct':                                       # V <= 255 and every call holds a news once: no two lengths of a call are equal
        return rng.permutation(V) + 1, rng.permutation(V) + 1
    assert kind == 'extremes'
    return rng.choice([1, 128], size=V), rng.choice([1, 128], size=V)


def _launch(hist, cand, tlen, clen, batch_size, first=0, count=None):
    from nnr_amd import ops
    dev = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda() for a in (hist, cand, tlen, clen)]
    outs = []
    for _ in range(2):
        outs.append([o.cpu().numpy() for o in ops.cne_pair_triples(*dev, batch_size, first, count)])
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes(), 'two launches differ'
    return outs[0]


# (samples, H, batch size): history calls of 1, 63, 64, 65 and 350 sequences next to candidate calls of 1 .. 65; a last batch of one sample
# (n = batch + 1, and 15 = 2 * 7 + 1); H = 1, and H = 50 / 13 / 9: no multiples of 64
SHAPES = [(1, 1, 1), (64, 1, 63), (65, 1, 64), (66, 1, 65), (15, 50, 7), (11, 13, 5), (131, 9, 65)]


@pytest.mark.parametrize('kind', ['random', 'tied', 'extremes'])
@pytest.mark.parametrize('n,H,B', SHAPES)
def test_plan_equals_the_restatement(n, H, B, kind):
    rng = np.random.default_rng(1000 * n + 10 * H + len(kind))
    V = 40
    tlen, clen = _lengths(kind, V, rng)
    hist, cand = rng.integers(0, V, size=(n, H)), rng.integers(0, V, size=n)
    got = _launch(hist, cand, tlen, clen, B)
    exp = R.pair_triples(hist, cand, tlen, clen, B)
    for name, g, e in zip(('pc_hist', 'pt_hist', 'pc_cand', 'pt_cand'), got, exp):
        assert g.dtype == np.int32 and g.shape == e.shape
        np.testing.assert_array_equal(g, e, err_msg='%s n %d H %d B %d %s' % (name, n, H, B, kind))
    if kind == 'tied':                                           # pure tie order: every sequence is its own partner
        np.testing.assert_array_equal(got[0], hist)
        np.testing.assert_array_equal(got[3], cand)


@pytest.mark.parametrize('n,H,B', [(5, 13, 5), (20, 1, 10), (9, 50, 5)])
def test_plan_without_ties(n, H, B):
    """All lengths of a call distinct: every call draws its news without replacement from 255 news of pairwise distinct lengths 1 .. 255
    (the top of the kernel's 256 bins)."""
    rng = np.random.default_rng(n + H)
    V = 255
    tlen, clen = _lengths('distinct', V, rng)
    hist, cand = np.zeros((n, H), dtype=np.int64), np.zeros(n, dtype=np.int64)
    for s in range(0, n, B):
        e = min(s + B, n)
        hist[s:e] = rng.permutation(V)[:(e - s) * H].reshape(e - s, H)
        cand[s:e] = rng.permutation(V)[:e - s]
    got = _launch(hist, cand, tlen, clen, B)
    for g, e in zip(got, R.pair_triples(hist, cand, tlen, clen, B)):
        np.testing.assert_array_equal(g, e)


def test_plan_of_a_split_that_repeats_one_impression_and_of_windows():
    """Every sample carries the same history row and the same candidate (repeated news: ties between copies of one news, which only their
    sequence index orders); windows of whole batches give the rows of the one launch over the whole split."""
    rng = np.random.default_rng(5)
    V, n, H, B = 25, 23, 10, 4
    tlen, clen = _lengths('random', V, rng)
    row = rng.integers(0, V, size=H)
    row[6:] = 0                                                  # PAD slots
    hist, cand = np.tile(row, (n, 1)), np.full(n, 3)
    whole = _launch(hist, cand, tlen, clen, B)
    for g, e in zip(whole, R.pair_triples(hist, cand, tlen, clen, B)):
        np.testing.assert_array_equal(g, e)
    hist2, cand2 = rng.integers(0, V, size=(n, H)), rng.integers(0, V, size=n)
    whole = _launch(hist2, cand2, tlen, clen, B)
    for first, count in ((0, 8), (8, 12), (20, 3), (4, 19), (16, 4)):
        part = _launch(hist2, cand2, tlen, clen, B, first, count)
        for w, g in zip(whole, part):
            np.testing.assert_array_equal(w[first:first + count], g)


def test_wrapper_refuses_ids_and_lengths_outside_the_tables():
    from nnr_amd import ops, _lib
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device='cuda')
    hist, cand, tlen, clen = i32([[0, 1], [2, 3]]), i32([1, 2]), i32([1, 2, 3, 4]), i32([4, 3, 2, 1])
    for args, word in (((i32([[0, 1], [2, 4]]), cand, tlen, clen), 'news ids'), ((hist, i32([-1, 2]), tlen, clen), 'news ids'),
                       ((hist, cand, i32([1, 2, 256, 4]), clen), 'lengths'), ((hist, cand, tlen, i32([4, -1, 2, 1])), 'lengths')):
        with pytest.raises(_lib.NnrHipError, match=word):
            ops.cne_pair_triples(*args, 2)
    assert all(o.numel() for o in ops.cne_pair_triples(hist, cand, tlen, clen, 2))


# ------------------------------------------------------------------------------------------------------------------ end to end
SIZES = np.array([5, 3, 6, 4, 5])                                # 23 samples: a last batch of 3 at batch size 4, of 7 at batch size 8
SEED = 0                                                         # Model.initialize()'s seed: the per-sample form's smallest gap is 6.8e-4 (CNE+ATT, batch 4)


def _config(news, user, **over):
    from nnr_amd.config import make_config
    return make_config(['--news_encoder=' + news, '--user_encoder=' + user, '--max_title_length=8', '--max_abstract_length=16', '--hidden_dim=16',
                        '--max_history_num=10', '--word_embedding_dim=48', '--attention_dim=16', '--category_embedding_dim=8',
                        '--subCategory_embedding_dim=8'], corpus_sizes=dict(vocabulary_size=300, category_num=5, subCategory_num=9),
                       tie_order='stable', **over)


@functools.lru_cache(maxsize=None)
def _split():
    """A dev-shaped split of five impressions whose consecutive samples share one history row, PAD slots included."""
    from nnr_amd.corpus import from_synth_lists
    from nnr_amd.synth import SynthSpec, SynthCorpus
    cfg = _config('CNE', 'ATT')
    synth = SynthCorpus(SynthSpec(vocabulary_size=cfg.vocabulary_size, category_num=cfg.category_num, subCategory_num=cfg.subCategory_num,
                                  max_title_length=cfg.max_title_length, max_abstract_length=cfg.max_abstract_length,
                                  max_history_num=cfg.max_history_num, news_pool=60, title_len_mean=4.0, content_len_mean=8.0, seed=9))
    dc = from_synth_lists(synth, SIZES, np.random.default_rng(21), 'cuda')
    mask = dc.t['beh_history_mask'].cpu().numpy()
    assert dc.num == int(SIZES.sum()) == 23 and not mask.all() and mask.any(), 'the split needs PAD slots and real history'
    o = 0
    for s in SIZES:                                              # consecutive samples share their history row
        assert bool((dc.t['beh_history'][o:o + s] == dc.t['beh_history'][o]).all())
        o += s
    labels = np.concatenate([(np.arange(s) == 1 % s).astype(np.uint8) for s in SIZES])
    return dc, labels


@functools.lru_cache(maxsize=None)
def _model_and_reference(news, user):
    """(model in train mode, {batch size: per-sample scores as numpy}): the reference form once per pair, then only read."""
    from nnr_amd import evaluate as E
    from nnr_amd.model import Model
    dc, _ = _split()
    torch.manual_seed(SEED)
    model = Model(_config(news, user))
    model.initialize()
    with torch.no_grad():                                        # M biases and proxy nodes are zero at init: make every path carry signal
        for p in model.parameters():
            if float(p.abs().max()) == 0.0:
                p.normal_(0, 0.05)
    model = model.cuda().train()
    ref = {}
    for bs in (4, 8):
        ref[bs] = E.compute_scores(model, dc, bs, cache=False).cpu().numpy()
        assert E.LAST_STATS['mode'] == 'per-sample'
    return model, ref


def _min_gap(scores):
    gaps, o = [], 0
    for s in SIZES:
        gaps.append(np.diff(np.sort(scores[o:o + s])).min())
        o += s
    return float(min(gaps))


@pytest.mark.parametrize('window', [1, 100])
@pytest.mark.parametrize('bs', [4, 8])
@pytest.mark.parametrize('news,user', [('CNE', 'SUE'), ('CNE', 'ATT'), ('CNE_wo_CA', 'ATT')])
def test_dedup_scores_are_the_per_sample_scores(news, user, bs, window):
    from nnr_amd import evaluate as E
    dc, labels = _split()
    model, ref = _model_and_reference(news, user)
    exp = ref[bs]
    gap, top = _min_gap(exp), float(np.abs(exp).max())
    got = E.compute_scores_dedup(model, dc, bs, window=window)
    st = dict(E.LAST_STATS)
    assert model.training, 'the model must come back in train mode'
    assert got.dtype == torch.float32 and tuple(got.shape) == exp.shape
    err = float(np.abs(got.cpu().numpy() - exp).max())
    t = dc.t
    tlen, clen = R.mask_lengths(t['news_title_mask'].cpu().numpy()), R.mask_lengths(t['news_abstract_mask'].cpu().numpy())
    hist, cand = t['beh_history'].cpu().numpy(), dc.samples[:, 0].cpu().numpy()
    want = R.distinct_triples(hist, cand, tlen, clen, bs, window)
    print('%s+%s batch %d window %d: |dedup - per-sample| %.3e (bar %.1e), max |score| %.3e, smallest gap %.3e, triples %d of %d rows, %d news'
          % (news, user, bs, window, err, BAR, top, gap, st['triples'], st['per_sample_rows'], st['distinct_news']))
    assert gap > 100 * BAR, 'an impression of the per-sample form is tied within 100 x the bar: choose another seed'
    assert top > 1e-3, 'degenerate scores would pass any bar'
    assert err <= BAR, (err, BAR)
    assert st['mode'] == 'dedup' and st['triples'] == want and st['triples'] < st['per_sample_rows'] == dc.num * (dc.H + 1)
    assert st['windows'] == -(-dc.num // (window * bs)) and st['distinct_news'] == np.unique(np.concatenate([hist.reshape(-1), cand])).size
    ranks, _, mean = E.rank_metrics(got, torch.from_numpy(labels), SIZES)
    eranks, _, emean = E.rank_metrics(torch.from_numpy(exp).cuda(), torch.from_numpy(labels), SIZES)
    assert torch.equal(ranks, eranks) and torch.equal(mean, emean)
    means, ranks2 = E.evaluate(model, dc, labels, SIZES, bs, dedup=True)
    assert E.LAST_STATS['mode'] == 'dedup' and torch.equal(ranks2, eranks)
    assert means == tuple(float(v) for v in emean.cpu())


def test_cacheable_and_default_paths_are_unchanged():
    from nnr_amd import evaluate as E
    dc, labels = _split()
    model, ref = _model_and_reference('CNE', 'ATT')
    E.evaluate(model, dc, labels, SIZES, 4)
    assert E.LAST_STATS['mode'] == 'per-sample'
    from nnr_amd.model import Model
    torch.manual_seed(1)
    cached = Model(_config('CNE_wo_CS', 'ATT'))
    cached.initialize()
    cached = cached.cuda()
    E.evaluate(cached, dc, labels, SIZES, 4, dedup=True)
    assert E.LAST_STATS['mode'] == 'cached'


def test_a_training_step_is_the_same_before_and_after_a_dedup_evaluation():
    """CNE in training mode, dropout on, forward and backward through the packed pair entry with the same seeds: the same bits before and
    after compute_scores_dedup -- the gate's table override lives on the evaluation's own calls and reaches no other."""
    from nnr_amd import evaluate as E
    from nnr_amd.corpus import from_synth
    from nnr_amd.model import Model
    from nnr_amd.synth import SynthSpec, SynthCorpus
    dc, _ = _split()
    cfg = _config('CNE', 'ATT', dropout_rate=0.2)
    torch.manual_seed(3)
    model = Model(cfg)
    model.initialize()
    model = model.cuda().train()
    ne = model.news_encoder
    synth = SynthCorpus(SynthSpec(vocabulary_size=cfg.vocabulary_size, category_num=cfg.category_num, subCategory_num=cfg.subCategory_num,
                                  max_title_length=cfg.max_title_length, max_abstract_length=cfg.max_abstract_length,
                                  max_history_num=cfg.max_history_num, news_pool=60, title_len_mean=4.0, content_len_mean=8.0, seed=9))
    train = from_synth(synth, 6, np.random.default_rng(2), 'cuda')
    g = torch.Generator().manual_seed(4)
    D = ne.news_embedding_dim
    douts = [torch.randn(6, 5, D, generator=g).cuda(), torch.randn(6, cfg.max_history_num, D, generator=g).cuda()]

    def step():
        b = train.train_batch(np.arange(6, dtype=np.int32))
        for p in ne.parameters():
            p.grad = None
        ne._calls = 0                                            # the same dropout seeds every time
        cand = (b[15], b[16], b[18], b[19], b[13], b[14])
        hist = (b[3], b[4], b[6], b[7], b[1], b[2])
        reps = list(ne.forward_pair(cand, hist))
        torch.autograd.backward(reps, douts)
        torch.cuda.synchronize()
        return [r.detach().clone() for r in reps] + [p.grad.clone() for p in ne.parameters()]

    before = step()
    again = step()
    for a, b in zip(before, again):
        assert torch.equal(a, b), 'the step itself is not reproducible'
    E.compute_scores_dedup(model, dc, 4, window=2)
    assert E.LAST_STATS['mode'] == 'dedup' and model.training
    after = step()
    assert len(after) == len(before) > 10
    for k, (a, b) in enumerate(zip(before, after)):
        assert torch.equal(a, b), 'tensor %d of the step changed after a dedup evaluation' % k
    assert float(before[0].abs().max()) > 0 and all(float(t.abs().max()) > 0 for t in before[2:4])
