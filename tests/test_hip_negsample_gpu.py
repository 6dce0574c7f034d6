"""The device negative sampler (csrc/corpus.hip: nnr_negative_sample) against its numpy restatement (tests/negsample_ref.py), bit for bit:
integer work, a pure function of (seed, epoch, behaviour).  The statistical quality of the construction is gated on the host
(tests/test_negsample_host.py); here the kernel is pinned to the restatement on every path: cyclic fill, random walk, padded rows, subset
calls, in-place redraws at a fixed address, record / replay on a launch tape, the DSSM corpus, and the refusals."""
import functools

import numpy as np
import pytest
import torch

import negsample_ref as R

pytestmark = pytest.mark.gpu
LENGTHS = (1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 300, 1000)
N_BEH = 5003             # not a multiple of the 256-thread block, nor of len(LENGTHS)
SENTINEL = -77


@functools.lru_cache(maxsize=None)
def _lists():
    """(clicks, neg_offsets, neg_ids) on the host and on the device: N_BEH behaviours, list lengths cycling through LENGTHS."""
    rng = np.random.default_rng(11)
    lens = np.asarray([LENGTHS[i % len(LENGTHS)] for i in range(N_BEH)], dtype=np.int64)
    off = np.zeros(N_BEH + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    host = (rng.integers(1, 10 ** 6, size=N_BEH).astype(np.int32), off, rng.integers(1, 10 ** 6, size=int(off[-1])).astype(np.int32))
    for a in host:
        a.setflags(write=False)
    return host, tuple(torch.tensor(a).cuda() for a in host)


@functools.lru_cache(maxsize=None)
def _want(K, seed, epoch):
    w = R.sample(*_lists()[0], K, seed, epoch)
    w.setflags(write=False)
    return w


def _call(table, K, seed, epoch, idx=None, n=None):
    from nnr_amd import _lib as L
    from nnr_amd.ops import _p, _s
    c, o, i = _lists()[1]
    n = (N_BEH if idx is None else idx.numel()) if n is None else n
    return L.lib().nnr_negative_sample(_p(c), _p(o), _p(i), _p(idx), n, K, seed, epoch, _p(table), table.shape[1], _s())


@pytest.mark.parametrize('seed,epoch', [(0, 0), (0xFEDCBA98, 37)])
@pytest.mark.parametrize('K,ld', [(4, 5), (1, 2), (8, 12)])
def test_table_equals_the_restatement_bit_for_bit(K, ld, seed, epoch):
    table = torch.full((N_BEH, ld), SENTINEL, device='cuda', dtype=torch.int32)
    assert _call(table, K, seed, epoch) == 0
    got = table.cpu().numpy()
    np.testing.assert_array_equal(got[:, :1 + K], _want(K, seed, epoch))
    assert (got[:, 1 + K:] == SENTINEL).all()                           # padding columns are not the sampler's


def test_subset_call_rewrites_exactly_its_rows():
    K, seed, epoch = 4, 3, 9
    sub = np.random.default_rng(2).permutation(N_BEH)[:257].astype(np.int32)
    table = torch.full((N_BEH, 1 + K), SENTINEL, device='cuda', dtype=torch.int32)
    assert _call(table, K, seed, epoch, idx=torch.from_numpy(sub).cuda()) == 0
    got = table.cpu().numpy()
    np.testing.assert_array_equal(got[sub], _want(K, seed, epoch)[sub])
    rest = np.ones(N_BEH, dtype=bool)
    rest[sub] = False
    assert (got[rest] == SENTINEL).all()


def test_refusals_write_nothing():
    from nnr_amd import _lib as L
    table = torch.full((N_BEH, 5), SENTINEL, device='cuda', dtype=torch.int32)
    wide = torch.full((N_BEH, 18), SENTINEL, device='cuda', dtype=torch.int32)
    assert _call(table, 0, 0, 0) == L.NNR_ERR_UNSUPPORTED
    assert _call(wide, 17, 0, 0) == L.NNR_ERR_UNSUPPORTED
    assert _call(table, 5, 0, 0) == L.NNR_ERR_ARG                       # ld_samples = 5 < 1 + K
    assert _call(table, 4, 0, 0, n=0) == L.NNR_ERR_ARG
    torch.cuda.synchronize()
    assert bool((table == SENTINEL).all()) and bool((wide == SENTINEL).all())


def _small_corpus(n_beh):
    from nnr_amd.corpus import from_synth
    from nnr_amd.synth import SynthSpec, SynthCorpus
    synth = SynthCorpus(SynthSpec(vocabulary_size=900, news_pool=500, max_history_num=8, max_title_length=8, max_abstract_length=16, seed=3))
    dc = from_synth(synth, n_beh, np.random.default_rng(4), 'cuda')
    rng = np.random.default_rng(5)
    beh = [(int(rng.integers(1, 500)), rng.integers(1, 500, size=LENGTHS[i % 9]).tolist()) for i in range(n_beh)]
    return synth, dc, R.csr(beh)


def _check_candidates(batch, synth, ids):
    np.testing.assert_array_equal(batch[13].cpu().numpy(), synth.category[ids])
    np.testing.assert_array_equal(batch[15].cpu().numpy(), synth.title_text[ids])
    np.testing.assert_array_equal(batch[18].cpu().numpy(), synth.content_text[ids])
    np.testing.assert_array_equal(batch[19].cpu().numpy(), synth.content_mask[ids])


def test_device_corpus_redraws_in_place_at_a_fixed_address():
    from nnr_amd import _lib as L
    synth, dc, csr = _small_corpus(301)
    with pytest.raises(L.NnrHipError):
        dc.sample_negatives(0)                                          # no impression lists yet
    with pytest.raises(ValueError):
        dc.set_impressions(csr[0][:-1], csr[1][:-1], csr[2][:csr[1][-2]])     # lists of 300 behaviours for a corpus of 301
    before = dc.resident_bytes()
    dc.set_impressions(*csr)
    assert dc.resident_bytes() == before + sum(a.nbytes for a in csr)    # the lists are resident too
    seen = {}
    for epoch in (0, 1, 2, 1):
        s = dc.sample_negatives(epoch, seed=6)
        assert s is dc.samples and s.shape == (301, 5) and s.dtype == torch.int32
        seen.setdefault('ptr', s.data_ptr())
        assert s.data_ptr() == seen['ptr']
        got = s.cpu().numpy()
        np.testing.assert_array_equal(got, R.sample(*csr, 4, 6, epoch))
        assert np.array_equal(seen.setdefault(epoch, got), got)         # epoch 1 again: identical bits
    assert not np.array_equal(seen[0], seen[1])
    idx = np.random.default_rng(6).permutation(301)[:37].astype(np.int32)
    _check_candidates(dc.train_batch(idx), synth, seen[1][idx])
    # a subset redraw for another epoch, indices given on the device: those rows move, the others stay
    sub = torch.from_numpy(idx[:9].copy()).cuda()
    dc.sample_negatives(2, seed=6, beh_idx=sub)
    want = seen[1].copy()
    want[idx[:9]] = seen[2][idx[:9]]
    np.testing.assert_array_equal(dc.samples.cpu().numpy(), want)
    with pytest.raises(L.NnrHipError):
        dc.sample_negatives(2, seed=6, beh_idx=[301])
    with pytest.raises(L.NnrHipError):
        dc.sample_negatives(2, seed=6, negative_sample_num=17)


def test_sampler_records_and_replays_on_a_tape_next_to_the_gather():
    """nnr_negative_sample + nnr_corpus_batch (+ nnr_history_graph) recorded once: `epoch` and `seed` are recorded arguments, so a replay
    redraws the RECORDED epoch, in place, and gathers the (patched) batch indices from it."""
    from nnr_amd.tape import Tape
    synth, dc, csr = _small_corpus(301)
    dc.set_impressions(*csr)
    dc.sample_negatives(0, seed=777777)                                 # allocates the table: first-use allocations are not tape material
    rng = np.random.default_rng(7)
    idx0, idx1 = (torch.from_numpy(rng.permutation(301)[:16].astype(np.int32)).cuda() for _ in range(2))
    sp = dc.sampler
    tape = Tape([idx0], {'news_seed': 1000, 'user_seed': 900000}, known=list(dc.t.values()) + [sp.clicks, sp.neg_offsets, sp.neg_ids, dc.samples])

    def body():
        dc.sample_negatives(2, seed=777777)
        return dc.train_batch(idx0)
    batch = tape.record(body)
    torch.cuda.synchronize()
    assert tape.violations == [] and tape.info()['calls'] == 3, (tape.violations, tape.info())
    table2 = R.sample(*csr, 4, 777777, 2)
    _check_candidates(batch, synth, table2[idx0.cpu().numpy()])
    ptr = dc.samples.data_ptr()
    dc.sample_negatives(5, seed=777777)                                 # the table moves on ...
    assert dc.samples.data_ptr() == ptr and not np.array_equal(dc.samples.cpu().numpy(), table2)
    tape.replay({'news_seed': 5000, 'user_seed': 1, 'adam_step': 1}, [idx1])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dc.samples.cpu().numpy(), table2)    # ... and the replay redraws the recorded epoch
    _check_candidates(batch, synth, table2[idx1.cpu().numpy()])
    tape.close()


def test_dssm_corpus_draws_on_the_device():
    from nnr_amd.dssm import DssmCorpus
    rng = np.random.default_rng(8)
    U, M, Lu, Ln, n = 40, 120, 12, 6, 203
    beh = [(int(rng.integers(0, U)), int(rng.integers(0, M)), rng.integers(0, M, size=LENGTHS[i % 8]).tolist()) for i in range(n)]
    corpus = DssmCorpus(rng.integers(0, 300, size=(U, Lu)), rng.random((U, Lu)), rng.integers(0, 300, size=(M, Ln)), rng.random((M, Ln)), 'cuda',
                        behaviors=beh)
    csr = R.csr([(c, neg) for _, c, neg in beh])
    for epoch in (0, 1):
        neg = corpus.negative_sampling_device(4, epoch, seed=12)
        assert neg is corpus.negatives
        np.testing.assert_array_equal(neg.cpu().numpy(), R.sample(*csr, 4, 12, epoch))
    ptr = corpus.negatives.data_ptr()
    assert corpus.negative_sampling_device(4, 2, seed=12).data_ptr() == ptr
    idx = torch.from_numpy(rng.permutation(n)[:33]).cuda()
    user_sel, news_sel = corpus.train_batch(idx)
    sel = idx.cpu().numpy()
    np.testing.assert_array_equal(user_sel.cpu().numpy(), np.asarray([u for u, _, _ in beh], dtype=np.int32)[sel])
    np.testing.assert_array_equal(news_sel.cpu().numpy(), R.sample(*csr, 4, 12, 2)[sel])
