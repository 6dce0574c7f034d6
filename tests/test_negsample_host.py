"""The device negative sampler (nnr_negative_sample, include/nnr_hip.h) on the host: its numpy restatement (tests/negsample_ref.py, which
the kernel equals bit for bit -- tests/test_hip_negsample_gpu.py) against the reference's rule (corpus.negative_sampling, MIND_dataset.py:
27-47) where no randomness is involved, its structural guarantees where it is, purity in (seed, epoch, behaviour), and a chi-square gate on
the generator.  Plus the host-side validation of the impression lists and the C-ABI surface of the new entry point."""
import itertools
import math

import numpy as np
import pytest

import negsample_ref as R

Z_GATE = 4.75            # one-sided p ~ 1e-6 per statistic: ~100 statistics together fail by chance about once in 1e4 (fixed seeds: deterministic)
N_GATE = 200000
PAIRS = [(0, 0), (0, 1), (7, 3), (1, 0)]


def chi2_bound(d, z=Z_GATE):
    """Chi-square quantile at normal deviate z, d degrees of freedom (Wilson-Hilferty)."""
    return d * (1 - 2 / (9 * d) + z * math.sqrt(2 / (9 * d))) ** 3


def chi2_columns(pos, m):
    """Per column: chi-square of the positions' counts against uniform over m cells (m - 1 degrees of freedom)."""
    e = pos.shape[0] / m
    return [float((((np.bincount(pos[:, j], minlength=m) - e) ** 2) / e).sum()) for j in range(pos.shape[1])]


def chi2_tuples(pos, m):
    """Chi-square of ordered K-tuples of positions against uniform over the m! / (m - K)! tuples without a repeat (which must carry all
    the mass)."""
    K = pos.shape[1]
    code = (pos * (m ** np.arange(K))[None, :]).sum(axis=1)
    legal = np.asarray([sum(v * m ** i for i, v in enumerate(t)) for t in itertools.permutations(range(m), K)])
    counts = np.bincount(code, minlength=m ** K)
    assert counts[legal].sum() == pos.shape[0], 'a tuple with a repeated position was drawn'
    e = pos.shape[0] / legal.shape[0]
    return float((((counts[legal] - e) ** 2) / e).sum()), legal.shape[0] - 1


def test_cyclic_fill_equals_the_host_sampler():
    """n <= K: no randomness; the restatement equals corpus.negative_sampling exactly (whatever seed / epoch)."""
    from nnr_amd.corpus import negative_sampling

    def no_draws(lo, hi):
        raise AssertionError('the cyclic fill draws nothing')
    for K, lens in ((4, (1, 2, 3, 4)), (1, (1,)), (8, (1, 2, 3, 4, 5, 6, 7, 8))):
        beh = [(100 + i, [1000 * (i + 1) + v for v in range(n)]) for i, n in enumerate(lens)]
        want = negative_sampling(beh, K, no_draws)
        for seed, epoch in PAIRS:
            got = R.sample(*R.csr(beh), K, seed, epoch)
            assert got.dtype == np.int32 and np.array_equal(got, want), (K, seed, epoch)


@pytest.mark.parametrize('K', [1, 4, 8, 16])
def test_random_rows_read_distinct_positions_of_their_own_list(K):
    rng = np.random.default_rng(K)
    lens = np.concatenate([np.arange(K + 1, K + 40), rng.integers(K + 1, 500, size=300)])
    beh, base = [], 0
    for i, n in enumerate(lens):
        beh.append((-(i + 1), list(range(base, base + n))))            # unique ids everywhere: an id names (behaviour, position)
        base += int(n)
    clicks, off, ids = R.csr(beh)
    s = R.sample(clicks, off, ids, K, 5, 2)
    assert np.array_equal(s[:, 0], clicks)
    pos = s[:, 1:] - off[:-1, None]
    assert (pos >= 0).all() and (pos < lens[:, None]).all()
    srt = np.sort(pos, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()
    assert np.array_equal(pos, R.positions(np.arange(len(beh)), lens, K, 5, 2))
    # one list with a repeated id: the POSITIONS are distinct, the ids need not be
    m = K + 3
    rep = [(9, [7] * m)] * 64
    assert (R.sample(*R.csr(rep), K, 0, 0)[:, 1:] == 7).all()
    p = R.positions(np.arange(64), m, K, 0, 0)
    assert all(len(set(row)) == K for row in p.tolist())


def test_pure_function_of_seed_epoch_and_behaviour():
    rng = np.random.default_rng(0)
    lens = rng.integers(1, 60, size=4000)
    beh = [(i, rng.integers(1, 10 ** 6, size=n).tolist()) for i, n in enumerate(lens)]
    c = R.csr(beh)
    K = 4
    full = R.sample(*c, K, 3, 5)
    assert np.array_equal(full, R.sample(*c, K, 3, 5))
    rnd = lens > 12                                                     # long enough that two draws rarely coincide by chance
    for seed, epoch in ((3, 6), (4, 5), (3 + 2 ** 32, 6)):
        other = R.sample(*c, K, seed, epoch)
        changed = (other[rnd] != full[rnd]).any(axis=1).mean()
        assert changed > 0.5, (seed, epoch, changed)
        assert np.array_equal(other[lens <= K], full[lens <= K])
    assert np.array_equal(R.sample(*c, K, 3 + 2 ** 32, 5), full)        # the seed is 32 bits wide
    sub = rng.permutation(4000)[:257]
    assert np.array_equal(R.sample(*c, K, 3, 5, beh_idx=sub), full[sub])


@pytest.mark.parametrize('m', [5, 7, 64, 300, 1000, 4096])
def test_uniformity_gate(m):
    """200 000 behaviours sharing one list of length m, K = 4: every column uniform over the m positions, and (m = 5, 7) the ordered 4-tuples
    uniform over the tuples without a repeat.  A generator that fails here is strengthened; the bound stays."""
    K = 4
    for seed, epoch in PAIRS:
        pos = R.positions(np.arange(N_GATE), m, K, seed, epoch)
        stats = chi2_columns(pos, m)
        print('m=%d seed=%d epoch=%d columns %s (bound %.1f)' % (m, seed, epoch, ['%.1f' % s for s in stats], chi2_bound(m - 1)))
        assert max(stats) < chi2_bound(m - 1), (m, seed, epoch, stats)
        if m <= 7:
            stat, dof = chi2_tuples(pos, m)
            print('    ordered 4-tuples %.1f at %d degrees of freedom (bound %.1f)' % (stat, dof, chi2_bound(dof)))
            assert dof == {5: 119, 7: 839}[m] and stat < chi2_bound(dof), (m, seed, epoch, stat)


@pytest.mark.parametrize('m', [5, 7])
def test_gate_threshold_passes_the_reference_sampler(m):
    """The same statistics on the reference's rejection sampler (corpus.negative_sampling over numpy.random.RandomState(0)) pass the same
    bound: the gate asks nothing of the device sampler that the host sampler does not deliver."""
    from nnr_amd.corpus import negative_sampling
    pos = negative_sampling([(0, list(range(m)))] * N_GATE, 4, np.random.RandomState(0).randint)[:, 1:].astype(np.int64)
    stats = chi2_columns(pos, m)
    stat, dof = chi2_tuples(pos, m)
    print('m=%d host sampler: columns %s (bound %.1f), 4-tuples %.1f (bound %.1f)' % (m, ['%.1f' % s for s in stats], chi2_bound(m - 1), stat, chi2_bound(dof)))
    assert max(stats) < chi2_bound(m - 1) and stat < chi2_bound(dof)


def test_impression_lists_are_validated_on_the_host():
    from nnr_amd.corpus import check_impressions, impression_lists
    beh = [(5, [7]), (6, [8, 9]), (1, [2, 3, 4, 10])]
    clicks, off, ids = impression_lists(beh)
    for got, want in zip((clicks, off, ids), R.csr(beh)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    c2, o2, i2 = check_impressions(clicks.astype(np.int64), off.tolist(), ids)
    assert (c2.dtype, o2.dtype, i2.dtype) == (np.int32, np.int64, np.int32) and np.array_equal(o2, off)
    with pytest.raises(ValueError, match='empty non-click list'):
        check_impressions(*impression_lists([(5, [7]), (6, []), (1, [2])]))
    with pytest.raises(ValueError, match='offsets'):
        check_impressions(clicks, off[:-1], ids)                        # one offset short
    with pytest.raises(ValueError, match='offsets'):
        check_impressions(clicks, off, ids[:-1])                        # the last offset points past the ids
    with pytest.raises(ValueError, match='offsets'):
        check_impressions(clicks, off + 1, ids)                         # does not start at 0
    with pytest.raises(ValueError, match='decreasing'):
        check_impressions(clicks, np.asarray([0, 3, 2, 7]), ids)


def test_cabi_surface_of_the_sampler():
    """Header, SIGNATURES and the tape registry agree on the new entry point (tests/test_cabi_exports.py compares every word); on a tape its
    seed names the run, not the step: recorded as a constant, like the epoch."""
    import torch
    from nnr_amd import _lib as L, tape as T
    assert L.SIGNATURES['nnr_negative_sample'] == 'i32 ptr ptr ptr ptr i32 i32 seed i32 ptr i32 stream'
    lib = L.lib()
    fid = lib.nnr_tape_fn_id(b'nnr_negative_sample')
    assert fid >= 0 and lib.nnr_tape_fn_nargs(fid) == 10
    name, index = next(iter(T.RUN_SEED_ARGS))
    assert L.kinds(name)[index] == 'seed'
    buf = torch.zeros(64)
    t = T.Tape([], {'news_seed': 1000, 'user_seed': 5000}, known=[buf])
    p = buf.data_ptr()
    slots, blobs, patches, violations = t.encode('nnr_negative_sample', (p, p + 8, p + 16, None, 3, 4, 777777, 2, p + 32, 5, None))
    assert slots == [p, p + 8, p + 16, 0, 3, 4, 777777, 2, p + 32, 5] and blobs == [] and patches == [] and violations == []
    assert t.encode('nnr_negative_sample', (p, p, p, None, 3, 4, 1003, 2, p, 5, None))[2] == []          # even next to a dropout seed
    # the sampler allocates nothing, so a recording may meet its first kept buffer AFTER its first call: that buffer is vouched for too
    first = torch.zeros(8)
    assert not t._vouched(first.data_ptr())
    t.keep.append(first)
    assert t._vouched(first.data_ptr())
    # refusals need no device: they are decided before any launch
    assert lib.nnr_negative_sample(p, p, p, None, 3, 0, 0, 0, p, 5, None) == L.NNR_ERR_UNSUPPORTED
    assert lib.nnr_negative_sample(p, p, p, None, 3, 17, 0, 0, p, 18, None) == L.NNR_ERR_UNSUPPORTED
    assert lib.nnr_negative_sample(p, p, p, None, 3, 4, 0, 0, p, 4, None) == L.NNR_ERR_ARG
    assert lib.nnr_negative_sample(p, p, p, None, 0, 4, 0, 0, p, 5, None) == L.NNR_ERR_ARG
    assert lib.nnr_negative_sample(None, p, p, None, 3, 4, 0, 0, p, 5, None) == L.NNR_ERR_ARG
