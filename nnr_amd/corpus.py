"""Device-resident corpus + id-only batches: the MI355X counterpart of MIND_Train_Dataset
(MIND_dataset.py:9-79) and of the pre-computed user-history graphs (MIND_corpus.py:162-221).

The reference keeps the corpus tables in host numpy arrays, fancy-indexes 21 arrays per sample in Python
(MIND_dataset.py:70-76) and ships 98.6 KB per impression over PCIe every step (trainer.py:83-103).  Here the tables are
uploaded once; a batch is (behaviour indices, sampled news ids) and two kernels of libnnr_hip.so fill the 21 tensors in HBM:
`nnr_corpus_batch` (row gather) and `nnr_history_graph` (graph / cluster mask / cluster indices from the history's
category ids -- the [behaviour lines, G, G] fp32 table, 18.5 KB per line, never exists).  No CPU fallback."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .ops import _p, _s

NORM = {'none': 0, 'symmetric': 1, 'asymmetric': 2, 'none_noself': 3}


def norm_from_config(config):
    """The graph normalisation the reference's flags select (config.py:56-58,111; MIND_corpus.py:180-214):
    --no_self_connection (only legal together with --no_adjacent_normalization) -> zero diagonal, no normalisation;
    --no_adjacent_normalization -> none; else --gcn_normalization_type ('symmetric' | 'asymmetric')."""
    if getattr(config, 'no_self_connection', False):
        assert getattr(config, 'no_adjacent_normalization', False), 'Adjacent normalization of graph only can be set in case of self-connection'
        return 'none_noself'
    if getattr(config, 'no_adjacent_normalization', False):
        return 'none'
    return getattr(config, 'gcn_normalization_type', 'symmetric')

_NEWS_KEYS = ('news_category', 'news_subCategory', 'news_title_text', 'news_title_mask', 'news_title_entity',
              'news_abstract_text', 'news_abstract_mask', 'news_abstract_entity')


def negative_sampling(behaviors, negative_sample_num, randint):
    """MIND_Train_Dataset.negative_sampling (MIND_dataset.py:27-47), host side: `behaviors` = [(click, [non-clicks]), ...],
    `randint(lo, hi)` the generator the reference draws from (numpy.random.randint).  Returns int32 [n, 1 + K]."""
    out = np.zeros((len(behaviors), 1 + negative_sample_num), dtype=np.int32)
    for i, (click, negatives) in enumerate(behaviors):
        out[i, 0] = click
        news_num = len(negatives)
        if news_num <= negative_sample_num:
            for j in range(negative_sample_num):
                out[i, j + 1] = negatives[j % news_num]
        else:
            used = set()
            for j in range(negative_sample_num):
                while True:
                    k = randint(0, news_num)
                    if k not in used:
                        out[i, j + 1] = negatives[k]
                        used.add(k)
                        break
    return out


NEG_K_MAX = 16           # nnr_negative_sample: 1 <= K <= 16


def impression_lists(behaviors):
    """[(click, [non-clicks]), ...] -> (clicks int32 [n], neg_offsets int64 [n + 1], neg_ids int32): the CSR form the device sampler reads."""
    clicks = np.asarray([c for c, _ in behaviors], dtype=np.int32)
    neg_offsets = np.zeros(len(behaviors) + 1, dtype=np.int64)
    np.cumsum([len(n) for _, n in behaviors], out=neg_offsets[1:])
    neg_ids = np.asarray([v for _, n in behaviors for v in n], dtype=np.int32)
    return clicks, neg_offsets, neg_ids


def check_impressions(clicks, neg_offsets, neg_ids):
    """Validate CSR impression lists on the host (the kernel trusts them) and return them as contiguous int32 / int64 / int32 arrays.
    An empty non-click list is refused: the reference's sampler divides by zero there (MIND_dataset.py:36)."""
    clicks = np.ascontiguousarray(clicks, dtype=np.int32).reshape(-1)
    neg_offsets = np.ascontiguousarray(neg_offsets, dtype=np.int64).reshape(-1)
    neg_ids = np.ascontiguousarray(neg_ids, dtype=np.int32).reshape(-1)
    n = clicks.shape[0]
    if n < 1 or neg_offsets.shape[0] != n + 1:
        raise ValueError('impression lists: %d clicks need %d offsets, got %d' % (n, n + 1, neg_offsets.shape[0]))
    if neg_offsets[0] != 0 or neg_offsets[-1] != neg_ids.shape[0]:
        raise ValueError('impression lists: offsets run from %d to %d, the non-click ids from 0 to %d'
                         % (neg_offsets[0], neg_offsets[-1], neg_ids.shape[0]))
    lens = np.diff(neg_offsets)
    if (lens <= 0).any():
        b = int(np.argmax(lens <= 0))
        raise ValueError('impression lists: behaviour %d has %s: nothing to sample from'
                         % (b, 'an empty non-click list' if lens[b] == 0 else 'decreasing offsets'))
    if int(lens.max()) >= 2 ** 31:
        raise ValueError('impression lists: a non-click list of %d entries (the sampler draws 32-bit positions)' % int(lens.max()))
    return clicks, neg_offsets, neg_ids


class NegativeSampler:
    """Impression lists in HBM + the sample table nnr_negative_sample writes: table[b] = (click, K sampled non-clicks) of behaviour b, a
    pure function of (seed, epoch, b) -- include/nnr_hip.h states the construction.  The table is allocated on the first draw and rewritten
    in place afterwards (same data_ptr() from epoch to epoch, as long as K stays), so a launch tape that recorded nnr_corpus_batch keeps
    reading the current epoch's samples.  Shared by DeviceCorpus and dssm.DssmCorpus."""

    def __init__(self, clicks, neg_offsets, neg_ids, device):
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise L.NnrHipError('NegativeSampler needs a GPU: the sampler lives in libnnr_hip.so (no CPU path)')
        clicks, neg_offsets, neg_ids = check_impressions(clicks, neg_offsets, neg_ids)
        self.device, self.num, self.table = dev, clicks.shape[0], None
        self.clicks, self.neg_offsets, self.neg_ids = (torch.from_numpy(a).to(dev) for a in (clicks, neg_offsets, neg_ids))

    def draw(self, epoch, seed=0, negative_sample_num=4, beh_idx=None):
        """Draw `epoch`'s samples of the behaviours `beh_idx` (int tensor on the device, or a sequence; None: all) into the table and return
        the table.  Recorded on a launch tape, `epoch` and `seed` are recorded arguments: a replay redraws the recorded epoch."""
        K = int(negative_sample_num)
        if not 1 <= K <= NEG_K_MAX:
            raise L.NnrHipError('negative_sample_num=%d: the device sampler draws 1..%d negatives' % (K, NEG_K_MAX))
        if self.table is None or self.table.shape[1] != 1 + K:
            if beh_idx is not None:
                raise L.NnrHipError('the first draw (of a given negative_sample_num) fills the whole table: beh_idx must be None')
            self.table = torch.empty((self.num, 1 + K), device=self.device, dtype=torch.int32)
        idx, n = None, self.num
        if beh_idx is not None:
            idx = beh_idx if torch.is_tensor(beh_idx) else torch.as_tensor(np.asarray(beh_idx), dtype=torch.int32)
            idx = idx.to(device=self.device, dtype=torch.int32).contiguous().reshape(-1)
            n = idx.numel()
            if n == 0:
                return self.table
            if int(idx.min()) < 0 or int(idx.max()) >= self.num:
                raise L.NnrHipError('beh_idx outside 0..%d' % (self.num - 1))
        L.check(L.lib().nnr_negative_sample(_p(self.clicks), _p(self.neg_offsets), _p(self.neg_ids), _p(idx), n, K, int(seed) & 0xFFFFFFFF,
                                            int(epoch), _p(self.table), 1 + K, _s()), 'nnr_negative_sample')
        return self.table


class DeviceCorpus:
    """Corpus tables in HBM. `arrays`: news_* tables [news(, T|C)], beh_user [n] int64, beh_history [n, H] int32 (news
    indices, 0 = PAD news), beh_history_mask [n, H] bool, optionally beh_line [n] + train_user_history_graph /
    _category_mask / _category_indices (the reference's pre-built tables; used when graph='table')."""

    def __init__(self, arrays, device, category_num, graph='build', norm='symmetric', config=None):
        if config is not None:                       # the reference's flags decide (they cannot disagree with a separate argument)
            norm = norm_from_config(config)
        assert graph in ('build', 'table') and norm in NORM
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise L.NnrHipError('DeviceCorpus needs a GPU: the batch kernels live in libnnr_hip.so (no CPU path)')
        self.device, self.graph_mode, self.norm, self.category_num = dev, graph, NORM[norm], int(category_num)
        self.norm_name = norm
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
        t = {}
        for k in _NEWS_KEYS:
            t[k] = up(arrays[k], torch.bool if k.endswith('mask') else torch.int32)
        t['beh_user'] = up(arrays['beh_user'], torch.int64)
        t['beh_history'] = up(arrays['beh_history'], torch.int32)
        t['beh_history_mask'] = up(arrays['beh_history_mask'], torch.bool)
        self.T, self.Cn = t['news_title_text'].shape[1], t['news_abstract_text'].shape[1]
        self.H = t['beh_history'].shape[1]
        self.G, self.K1 = self.H + self.category_num, self.category_num + 1
        if graph == 'table':
            t['beh_line'] = up(arrays['beh_line'], torch.int32)
            t['graph_table'] = up(arrays['train_user_history_graph'], torch.float32)
            t['cmask_table'] = up(arrays['train_user_history_category_mask'], torch.bool)
            t['cidx_table'] = up(arrays['train_user_history_category_indices'], torch.int64)
            assert t['graph_table'].shape[1] == self.G
        self.t = t
        self.num = t['beh_user'].shape[0]
        self.samples = None
        self.sampler = None
        ct = L.CorpusTables()
        ct.news_category, ct.news_subCategory = _p(t['news_category']), _p(t['news_subCategory'])
        ct.title_text, ct.title_mask, ct.title_entity = _p(t['news_title_text']), _p(t['news_title_mask']), _p(t['news_title_entity'])
        ct.abstract_text, ct.abstract_mask, ct.abstract_entity = _p(t['news_abstract_text']), _p(t['news_abstract_mask']), _p(t['news_abstract_entity'])
        ct.beh_user, ct.beh_history, ct.beh_history_mask = _p(t['beh_user']), _p(t['beh_history']), _p(t['beh_history_mask'])
        ct.beh_line, ct.graph_table, ct.cmask_table, ct.cidx_table = _p(t.get('beh_line')), _p(t.get('graph_table')), _p(t.get('cmask_table')), _p(t.get('cidx_table'))
        ct.T, ct.C, ct.H, ct.G, ct.K1 = self.T, self.Cn, self.H, self.G, self.K1
        self._ct = ct

    def set_samples(self, samples):
        """[behaviours, 1 + K] news ids: column 0 the clicked news, the rest the sampled non-clicks (`negative_sampling`)."""
        self.samples = torch.as_tensor(np.ascontiguousarray(samples), dtype=torch.int32).to(self.device)
        assert self.samples.shape[0] == self.num

    def set_impressions(self, clicks, neg_offsets, neg_ids):
        """Upload, once, every behaviour's click and non-click list (CSR, impression_lists' layout) for sample_negatives()."""
        sampler = NegativeSampler(clicks, neg_offsets, neg_ids, self.device)
        if sampler.num != self.num:
            raise ValueError('impression lists of %d behaviours for a corpus of %d' % (sampler.num, self.num))
        self.sampler = sampler

    def sample_negatives(self, epoch, seed=0, negative_sample_num=4, beh_idx=None):
        """This epoch's samples, drawn on the device (NegativeSampler.draw): `self.samples` is allocated on first use and rewritten in place
        afterwards (same data_ptr() across epochs); `beh_idx` redraws only those rows.  Returns self.samples."""
        if self.sampler is None:
            raise L.NnrHipError('call set_impressions() before sample_negatives()')
        self.samples = self.sampler.draw(epoch, seed, negative_sample_num, beh_idx)
        return self.samples

    def resident_bytes(self):
        lists = (self.sampler.clicks, self.sampler.neg_offsets, self.sampler.neg_ids) if self.sampler is not None else ()
        return (sum(v.numel() * v.element_size() for v in list(self.t.values()) + list(lists))
                + (self.samples.numel() * 4 if self.samples is not None else 0))

    def train_batch(self, beh_idx):
        """The 21 tensors of trainer.py:105-106 for the behaviours `beh_idx` (int32 tensor on the device, or a sequence)."""
        if self.samples is None:
            raise L.NnrHipError('call set_samples() (negative sampling) before train_batch()')
        idx = beh_idx if torch.is_tensor(beh_idx) else torch.as_tensor(np.asarray(beh_idx), dtype=torch.int32)
        idx = idx.to(device=self.device, dtype=torch.int32).contiguous()
        B, S, H, T, Cn, G, K1, dev = idx.numel(), self.samples.shape[1], self.H, self.T, self.Cn, self.G, self.K1, self.device
        e = lambda shape, dt: torch.empty(shape, device=dev, dtype=dt)
        out = [e((B,), torch.int64),
               e((B, H), torch.int32), e((B, H), torch.int32), e((B, H, T), torch.int32), e((B, H, T), torch.bool), e((B, H, T), torch.int32),
               e((B, H, Cn), torch.int32), e((B, H, Cn), torch.bool), e((B, H, Cn), torch.int32),
               e((B, H), torch.bool), e((B, G, G), torch.float32), e((B, K1), torch.bool), e((B, H), torch.int64),
               e((B, S), torch.int32), e((B, S), torch.int32), e((B, S, T), torch.int32), e((B, S, T), torch.bool), e((B, S, T), torch.int32),
               e((B, S, Cn), torch.int32), e((B, S, Cn), torch.bool), e((B, S, Cn), torch.int32)]
        bo = L.BatchOut()
        for (name, _), ten in zip(L.BatchOut._fields_, out):
            setattr(bo, name, _p(ten))
        L.check(L.lib().nnr_corpus_batch(C.byref(self._ct), C.byref(bo), _p(idx), _p(self.samples), S, B, S, _s()), 'nnr_corpus_batch')
        if self.graph_mode == 'build':
            L.check(L.lib().nnr_history_graph(_p(out[1]), _p(out[9]), B, H, self.category_num, self.norm, _p(out[10]), _p(out[11]), _p(out[12]),
                                              _s()), 'nnr_history_graph')
        return out


def history_graph(cats, hmask, category_num, norm='symmetric'):
    """Graph / cluster mask / cluster indices for a batch from category ids [B, H] int32 and the history mask [B, H] bool."""
    B, H = cats.shape
    G = H + category_num
    graph = torch.empty((B, G, G), device=cats.device, dtype=torch.float32)
    cmask = torch.empty((B, category_num + 1), device=cats.device, dtype=torch.bool)
    cidx = torch.empty((B, H), device=cats.device, dtype=torch.int64)
    L.check(L.lib().nnr_history_graph(_p(cats.contiguous()), _p(hmask.contiguous()), B, H, category_num, NORM[norm], _p(graph), _p(cmask), _p(cidx),
                                      _s()), 'nnr_history_graph')
    return graph, cmask, cidx


def from_synth(synth, n_behaviors, rng, device, graph='build'):
    """A DeviceCorpus over a SynthCorpus news pool with `n_behaviors` synthetic behaviours (bench / tests)."""
    s = synth.spec
    H, S = s.max_history_num, 1 + s.negative_sample_num
    counts = rng.integers(0, H + 1, size=n_behaviors)
    counts[rng.random(n_behaviors) < s.empty_history_frac] = 0
    hist = np.zeros((n_behaviors, H), dtype=np.int32)
    hmask = np.arange(H)[None, :] < counts[:, None]
    for b in range(n_behaviors):
        hist[b, :counts[b]] = rng.integers(1, s.news_pool, size=counts[b])
    arrays = dict(news_category=synth.category, news_subCategory=synth.subCategory, news_title_text=synth.title_text,
                  news_title_mask=synth.title_mask, news_title_entity=synth.title_entity, news_abstract_text=synth.content_text,
                  news_abstract_mask=synth.content_mask, news_abstract_entity=synth.content_entity,
                  beh_user=np.arange(n_behaviors, dtype=np.int64), beh_history=hist, beh_history_mask=hmask)
    if graph == 'table':
        g = [synth.history_graph(synth.category[hist[b]], int(counts[b])) for b in range(n_behaviors)]
        arrays.update(beh_line=np.arange(n_behaviors, dtype=np.int32), train_user_history_graph=np.stack([x[0] for x in g]),
                      train_user_history_category_mask=np.stack([x[1] for x in g]), train_user_history_category_indices=np.stack([x[2] for x in g]))
    dc = DeviceCorpus(arrays, device, s.category_num, graph=graph)
    dc.set_samples(rng.integers(1, s.news_pool, size=(n_behaviors, S)).astype(np.int32))
    return dc


def from_synth_lists(synth, sizes, rng, device, distinct_users=None):
    """A dev-shaped DeviceCorpus over a SynthCorpus news pool (bench / tests): impression i is sizes[i] contiguous (impression, candidate)
    samples that repeat one behaviour row (user, history, mask), each with one candidate drawn from the pool.  distinct_users: the
    impressions draw their behaviour row from that many distinct rows (a user's history is the same in all their impressions of a split);
    None: one row per impression."""
    s = synth.spec
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    H, n_rows = s.max_history_num, int(distinct_users or sizes.size)
    counts = rng.integers(0, H + 1, size=n_rows)
    counts[rng.random(n_rows) < s.empty_history_frac] = 0
    hist = np.zeros((n_rows, H), dtype=np.int32)
    hmask = np.arange(H)[None, :] < counts[:, None]
    for b in range(n_rows):
        hist[b, :counts[b]] = rng.integers(1, s.news_pool, size=counts[b])
    owner = np.arange(sizes.size, dtype=np.int64) if distinct_users is None else rng.integers(0, n_rows, size=sizes.size)
    beh = np.repeat(owner, sizes)
    arrays = dict(news_category=synth.category, news_subCategory=synth.subCategory, news_title_text=synth.title_text,
                  news_title_mask=synth.title_mask, news_title_entity=synth.title_entity, news_abstract_text=synth.content_text,
                  news_abstract_mask=synth.content_mask, news_abstract_entity=synth.content_entity,
                  beh_user=beh, beh_history=hist[beh], beh_history_mask=hmask[beh])
    dc = DeviceCorpus(arrays, device, s.category_num)
    dc.set_samples(rng.integers(1, s.news_pool, size=(beh.size, 1)).astype(np.int32))
    return dc
