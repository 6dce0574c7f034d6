"""Evaluation path on the device: util.compute_scores (util.py:10-68) + evaluate.scoring
(evaluate.py:32-89).  Dev / test samples are (impression, candidate) pairs; the model scores each with news_num = 1
(util.py:43-50), candidates are ranked inside their impression and AUC / MRR / nDCG@5 / nDCG@10 are averaged over
impressions.  Batches come from a DeviceCorpus (id-only), scores never leave HBM until the four means are read back."""
import contextlib

import numpy as np
import torch

from . import _lib as L
from . import ops
from .corpus import DeviceCorpus, history_graph
from .ops import _p, _s


def dev_corpus(arrays, device, category_num, graph='build', norm='symmetric'):
    """DeviceCorpus over dev / test behaviours (MIND_corpus.py:355-371): `arrays` as for DeviceCorpus plus beh_candidate [n]."""
    dc = DeviceCorpus(arrays, device, category_num, graph=graph, norm=norm)
    dc.set_samples(np.asarray(arrays['beh_candidate'], dtype=np.int32).reshape(-1, 1))
    return dc


LAST_STATS = {}          # filled by compute_scores: how many news rows the news encoder processed (cached / per-sample / listwise / dedup form), or what recommend ranked


def news_reps_cacheable(model):
    """A news representation may be cached (encoded once per evaluation, gathered by id) only if it does not depend on the
    other news of its encoder call.  True for the MHSA / CNN encoders; NOT for CNE: the reference gates the title at
    title-rank r with the content memory at content-rank r of the SAME call (newsEncoders.py:112-115,128-129), so its
    representations depend on their batch-mates and caching would change the reference's scores."""
    return model.news_encoder.batch_independent and hasattr(model.user_encoder, 'encode_user')


@contextlib.contextmanager
def eval_mode(model):
    """`model` in eval mode for the body; the mode it had before comes back however the body ends."""
    was_training = model.training
    model.eval()
    try:
        yield model
    finally:
        model.train(was_training)


@torch.no_grad()
def encode_news_table(model, corpus, ids, chunk=4096):
    """Representations [len(ids), D] of the news `ids` (int64 device tensor of news indices), chunk by chunk, eval mode."""
    t = corpus.t
    ne = model.news_encoder
    out = torch.empty((ids.numel(), ne.news_embedding_dim), device=corpus.device, dtype=torch.float32)
    for s in range(0, ids.numel(), chunk):
        sel = ids[s:s + chunk]
        f = lambda k: t[k][sel].unsqueeze(1).contiguous()          # [n, 1, ...]: one news per "sample"
        rep = ne(f('news_title_text'), f('news_title_mask'), f('news_title_entity'), f('news_abstract_text'), f('news_abstract_mask'),
                 f('news_abstract_entity'), f('news_category'), f('news_subCategory'), None)
        out[s:s + sel.numel()] = rep.view(sel.numel(), -1)
    return out


# ------------------------------------------------------------------------------------------------ what the table-driven paths share
def _split_like(inv, groups):
    """The inverse of a unique over the concatenated, flattened `groups`, cut back into one tensor per group, each in its group's shape."""
    out, o = [], 0
    for g in groups:
        out.append(inv[o:o + g.numel()].view_as(g))
        o += g.numel()
    return out


def _news_table(model, corpus, *groups):
    """(used, reps, slots): the distinct news of the int64 index tensors `groups`, ascending, each encoded once (row i of reps = news used[i]),
    and per group the rows of reps of its news, in the group's shape."""
    used, inv = torch.unique(torch.cat([g.reshape(-1) for g in groups]), return_inverse=True)
    return used, encode_news_table(model, corpus, used), _split_like(inv, groups)


def _distinct_rows(users, hist, hmask):
    """(users int64 [R], hist int64 [R, H], hmask bool [R, H], back int64 [n]): the distinct (user, history, mask) rows of n behaviour rows in
    sorted order, and for every input row its distinct row."""
    H = hist.shape[1]
    key, back = torch.unique(torch.cat([users.view(-1, 1), hist.long(), hmask.long()], dim=1), dim=0, return_inverse=True)
    return key[:, 0].contiguous(), key[:, 1:1 + H], key[:, 1 + H:] != 0, back


def _encoded_users(model, corpus, reps, users, hist, hmask, slot_h, slot_cand, batch_size):
    """The user encoder over R behaviour rows (users [R], hist [R, H] news indices, hmask [R, H]; slot_h [R, H]: the rows of `reps` of the
    history news), `batch_size` rows per encode_user call in eval mode: yields (s, e, user [e - s, K, D], c) for rows s .. e - 1.  slot_cand
    int64 [R, K]: the rows of `reps` of K candidates per row, c = their representations [e - s, K, D]; None: c is a blank [e - s, 1, D] that
    candidate_independent encoders never read.  Per batch: the gathers, then the graph / cluster inputs for the encoders that read them (SUE
    and its ablations), then the user rows where the model has a user table (without dropout), then encode_user."""
    R, ue = users.numel(), model.user_encoder
    blank = torch.zeros((min(batch_size, R), 1, reps.shape[1]), device=corpus.device, dtype=torch.float32) if slot_cand is None else None
    for s in range(0, R, batch_size):
        e = min(s + batch_size, R)
        h = reps[slot_h[s:e]]                                                  # [r, H, D]
        c = blank[:e - s] if slot_cand is None else reps[slot_cand[s:e]]       # [r, 1, D] (never read) / [r, K, D]
        m = hmask[s:e].contiguous()
        graph = cmask = cidx = None
        if ue.needs_history_graph:
            graph, cmask, cidx = history_graph(corpus.t['news_category'][hist[s:e].long()].contiguous(), m, corpus.category_num, corpus.norm_name)
        rows = model.user_rows(users[s:e].long()) if model.use_user_embedding else None
        yield s, e, model._encode_user(rows, h, m, graph, cmask, cidx, c), c


@torch.no_grad()
def compute_scores_cached(model, corpus, batch_size):
    """compute_scores for encoders with batch-independent news representations (the reference's README
    lists the missing cache as a known cost, README.md:125): every DISTINCT news of the split is encoded once, a sample's history
    / candidate representations are gathered by news id, and only the user encoder + click predictor run per sample."""
    from .model import _DotProductFn
    assert news_reps_cacheable(model)
    t = corpus.t
    hist, cand = t['beh_history'].long(), corpus.samples[:, 0].long()
    scores = torch.zeros(corpus.num, device=corpus.device, dtype=torch.float32)
    with eval_mode(model):
        used, reps, (slot_h, slot_c) = _news_table(model, corpus, hist, cand.view(-1, 1))
        for s, e, user, c in _encoded_users(model, corpus, reps, t['beh_user'], hist, t['beh_history_mask'], slot_h, slot_c, batch_size):
            scores[s:e] = _DotProductFn.apply(user, c).squeeze(dim=1)
    LAST_STATS.update(mode='cached', encoder_rows=int(used.numel()), per_sample_rows=int(corpus.num * (hist.shape[1] + 1)))
    return scores


@torch.no_grad()
def compute_scores(model, corpus, batch_size, cache='auto'):
    """One score per dev sample, in dataset order (util.py:13-49): float32 [n] on the device.  cache: 'auto' (cache the news
    representations when the encoder allows it, see news_reps_cacheable), True, False (the reference's per-sample form)."""
    if cache is True or (cache == 'auto' and news_reps_cacheable(model)):
        return compute_scores_cached(model, corpus, batch_size)
    model.news_encoder.__dict__['_dedup_stats'] = [0, 0]
    scores = torch.zeros(corpus.num, device=corpus.device, dtype=torch.float32)
    with eval_mode(model):
        for start in range(0, corpus.num, batch_size):
            idx = torch.arange(start, min(start + batch_size, corpus.num), device=corpus.device, dtype=torch.int32)
            batch = corpus.train_batch(idx)                       # candidate fields are [B, 1, ...] = the unsqueeze of util.py:43-48
            scores[start:start + idx.numel()] = model(*batch).squeeze(dim=1)
    rows = int(corpus.num * (corpus.H + 1))
    enc, of = model.news_encoder.__dict__.get('_dedup_stats', [0, 0])
    # CNE: history slots whose representation is the constant PAD representation are not encoded (news_encoders.cne_history_dedup)
    LAST_STATS.update(mode='per-sample', encoder_rows=rows - (of - enc), per_sample_rows=rows, pad_slots_skipped=of - enc)
    return scores


# ------------------------------------------------------------------------------------------------ listwise evaluation
# All candidates of an impression share one user and one history, so the user encoder needs to run once per impression, not once per
# (impression, candidate) sample.  Two modes, by what the encoder reads:
#   candidate_independent (ATT, MHSA, GRU, PUE, SUE_wo_HCA): ONE user vector per impression (or per distinct user row), whatever the candidates.
#   candidate-aware (SUE, SUE_wo_GCN, CATT, OMAP): an impression's candidates go through encode_user K at a time -- a row of K candidates is a
#   training-shaped sample with news_num = K -- and every candidate's user vector depends on its own candidate only.
# Either way the scores are one nnr_list_scores launch over (user row, candidate row) pairs.
class ListPlan:
    """Where every sample of a split sits (list_plan).  n samples, R user rows of K slots:
      imp int64 [n]           the impression of sample j
      first int64 [n_imp]     the impression's first sample
      row_imp int64 [R]       the impression of row r
      row_slots int64 [R, K]  the sample in slot k of row r; a pad slot holds the row's first sample   (candidate-aware mode only,
      slot_valid bool [R, K]  False for a pad slot                                                     None in the independent mode)
      row int32 [n]           the slot of sample j, r * K + k; in the independent mode the row itself = the impression of sample j"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def list_plan(sizes, candidates_per_row=None):
    """The row / slot layout of listwise evaluation for impressions of `sizes` contiguous samples each (host, numpy).  candidates_per_row=None:
    one row per impression (independent mode); K: impression i takes ceil(size_i / K) rows of K slots, filled in sample order."""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    if sizes.size < 1 or int(sizes.min()) < 1:
        raise ValueError('list_plan: every impression needs at least one candidate')
    K = 1 if candidates_per_row is None else int(candidates_per_row)
    if K < 1:
        raise ValueError('list_plan: candidates_per_row=%d' % K)
    n_imp, n = sizes.size, int(sizes.sum())
    first = np.zeros(n_imp, dtype=np.int64)
    np.cumsum(sizes[:-1], out=first[1:])
    imp = np.repeat(np.arange(n_imp, dtype=np.int64), sizes)
    if candidates_per_row is None:
        row_first = row_imp = np.arange(n_imp, dtype=np.int64)
        pos = np.zeros(n, dtype=np.int64)                              # every sample of an impression reads the impression's one row
        row_slots = slot_valid = None                                  # no slots: a row serves every sample of its impression
    else:
        rows_of = (sizes + K - 1) // K
        row_first = np.zeros(n_imp, dtype=np.int64)
        np.cumsum(rows_of[:-1], out=row_first[1:])
        pos = np.arange(n, dtype=np.int64) - first[imp]                # position inside the impression
        row_imp = np.repeat(np.arange(n_imp, dtype=np.int64), rows_of)
        in_imp = (np.arange(row_imp.size, dtype=np.int64) - row_first[row_imp])[:, None] * K + np.arange(K, dtype=np.int64)[None, :]
        slot_valid = in_imp < sizes[row_imp][:, None]
        head = first[row_imp] + in_imp[:, 0]                           # the row's first sample: what a pad slot holds
        row_slots = np.where(slot_valid, first[row_imp][:, None] + in_imp, head[:, None])
    row = row_first[imp] * K + pos
    if row.size and int(row.max()) >= 2 ** 31:
        raise ValueError('list_plan: %d slots do not fit the kernel\'s int32 row indices' % (int(row.max()) + 1))
    return ListPlan(n=n, K=K, candidates_per_row=candidates_per_row, imp=imp, first=first, row_imp=row_imp, row_slots=row_slots,
                    slot_valid=slot_valid, row=row.astype(np.int32))


LISTWISE_REFUSAL = ('listwise evaluation needs news representations that do not depend on their batch-mates (news_reps_cacheable): %s is not '
                    'batch_independent -- the reference pairs the news of one encoder call, so scoring an impression as a list would change its scores')


def listwise_supported(model):
    """Listwise evaluation gathers every representation from the table of distinct news: the rule is news_reps_cacheable's."""
    return news_reps_cacheable(model)


def _check_lists(t, plan, dev):
    """Every sample's (user, history, mask) row equals its impression's first sample's: one device reduction, one sync."""
    fs = torch.from_numpy(plan.first[plan.imp]).to(dev)
    same = ((t['beh_user'] == t['beh_user'][fs]).all() & (t['beh_history'] == t['beh_history'][fs]).all()
            & (t['beh_history_mask'] == t['beh_history_mask'][fs]).all())
    if not bool(same):
        raise ValueError('listwise evaluation: a sample\'s user, history or history mask differs from its impression\'s first sample '
                         '(sizes must delimit impressions whose samples share one behaviour row)')


@torch.no_grad()
def _user_table(model, corpus, reps, users, hist, hmask, slot_h, slot_cand, batch_size):
    """The user vectors [R * K, D] of R behaviour rows (users [R], hist int64 [R, H], hmask [R, H]; slot_h [R, H]: the rows of `reps` of the
    history news), `batch_size` rows per encode_user call.  slot_cand None: one vector per row (candidate_independent encoders, which never
    read the candidates); int64 [R, K]: the rows of `reps` of K candidates per row, one vector per candidate."""
    R, D = users.numel(), reps.shape[1]
    K = 1 if slot_cand is None else slot_cand.shape[1]
    table = torch.empty((R * K, D), device=corpus.device, dtype=torch.float32)
    for s, e, user, _ in _encoded_users(model, corpus, reps, users, hist, hmask, slot_h, slot_cand, batch_size):
        table[s * K:e * K] = user.reshape((e - s) * K, D)
    return table


@torch.no_grad()
def compute_scores_listwise(model, corpus, sizes, batch_size, candidates_per_row=8, dedup_users=True, check=True):
    """One score per dev sample in dataset order, float32 [n] on the device, as compute_scores -- with the user encoder run once per
    impression (candidate_independent encoders; once per distinct (user, history, mask) row with dedup_users) or once per row of
    `candidates_per_row` candidates of one impression (candidate-aware encoders), and ONE nnr_list_scores launch for all scores.
    `sizes`: candidates per impression (contiguous, file order).  check=True verifies that the samples of an impression share their behaviour
    row.  Refused (NnrHipError naming the reason) for encoders whose news representations cannot be cached."""
    if not listwise_supported(model):
        raise L.NnrHipError(LISTWISE_REFUSAL % type(model.news_encoder).__name__)
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    if int(sizes.sum()) != corpus.num:
        raise ValueError('listwise evaluation: sizes sum to %d, the corpus holds %d samples' % (int(sizes.sum()), corpus.num))
    independent = model.user_encoder.candidate_independent
    plan = list_plan(sizes, None if independent else candidates_per_row)
    t, dev = corpus.t, corpus.device
    if check:
        _check_lists(t, plan, dev)
    with eval_mode(model):
        first = torch.from_numpy(plan.first).to(dev)
        row = torch.from_numpy(plan.row).to(dev)
        if independent:
            users, hist, hmask = t['beh_user'][first], t['beh_history'][first], t['beh_history_mask'][first]
            if dedup_users:
                users, hist, hmask, back = _distinct_rows(users, hist, hmask)
                row = back[torch.from_numpy(plan.imp).to(dev)].to(torch.int32)
            slots = None
        else:
            rf = first[torch.from_numpy(plan.row_imp).to(dev)]                      # a row reads its impression's behaviour row
            users, hist, hmask = t['beh_user'][rf], t['beh_history'][rf], t['beh_history_mask'][rf]
            slots = torch.from_numpy(plan.row_slots).to(dev)
        R = users.numel()
        hist = hist.long()
        used, reps, (slot_h, slot_c) = _news_table(model, corpus, hist, corpus.samples[:, 0].long())
        table = _user_table(model, corpus, reps, users, hist, hmask, slot_h, None if independent else slot_c[slots], batch_size)
        scores = ops.list_scores(table, reps, row.contiguous(), slot_c.to(torch.int32).contiguous(), check=check)
    LAST_STATS.update(mode='listwise', user_rows=int(R), per_sample_user_rows=int(corpus.num), encoder_rows=int(used.numel()),
                      candidates_per_row=plan.candidates_per_row)
    return scores


# ------------------------------------------------------------------------------------------------ top-K recommendation
# Every form above scores (impression, candidate) pairs that the behaviours file chose.  recommend answers the other question: the K news of
# a pool that the model ranks highest for a user.  With cacheable news representations, ONE user vector per row and the dot-product head
# that is [users, D] x [news, D] -> [users, K], which nnr_topk_scores computes without the [users, news] scores ever existing.
# OMAP is candidate-aware only behind its K archives (pool_archives): the same product once per archive, combined per pair (nnr_topk_archive_scores).
def recommend_refusal(model, archives=False):
    """None when recommend can serve `model`, else the reason it cannot.  archives: the caller's `archives` keyword -- True admits a
    pool_archives user encoder (OMAP), whose pool is ranked on its candidate-free archives; False, the default, keeps the answer recommend
    has always given for it."""
    ne, ue = model.news_encoder, model.user_encoder
    if getattr(model, 'click_predictor', 'dot_product') != 'dot_product':
        return ('recommend ranks a pool by inner products of one user vector with the news representations (the dot_product click predictor): '
                'this model\'s click predictor is %s' % model.click_predictor)
    if not news_reps_cacheable(model):
        return LISTWISE_REFUSAL % type(ne).__name__
    if not ue.candidate_independent and not (archives and ue.pool_archives):
        return ('recommend needs ONE user vector per behaviour row (candidate_independent: ATT, MHSA, GRU, PUE, SUE_wo_HCA) or, with '
                'archives=True, candidate-free archives whose inner products give the score (pool_archives: OMAP): the user vector of %s is a '
                'function of the candidate, so a pool-wide search would need one encoder run per (user, news)%s'
                % (type(ue).__name__, ' -- unless it is ranked on its archives: pass archives=True' if ue.pool_archives else ''))
    return None


def _index_list(what, x, hi, dev, name='recommend'):
    """`x` as an int64 device vector of indices in 0 .. hi - 1 (ValueError otherwise; one sync)."""
    x = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(device=dev, dtype=torch.int64).reshape(-1)
    if x.numel() and not (0 <= int(x.min()) and int(x.max()) < hi):
        raise ValueError('%s: %s %d..%d outside 0..%d' % (name, what, int(x.min()), int(x.max()), hi - 1))
    return x


def _pool_rows(name, corpus, rows, pool):
    """(rows, pool, V) of recommend / rank_in_pool as int64 device vectors: the behaviour rows (default: all) and the distinct pool news in
    ascending order (default: every news of the corpus but PAD news 0)."""
    t, dev = corpus.t, corpus.device
    V = t['news_title_mask'].shape[0]
    rows = torch.arange(t['beh_user'].shape[0], device=dev) if rows is None else _index_list('rows', rows, t['beh_user'].shape[0], dev, name)
    pool = torch.arange(1, V, device=dev) if pool is None else torch.unique(_index_list('pool news', pool, V, dev, name))
    if rows.numel() < 1:
        raise ValueError('%s: no rows' % name)
    return rows, pool, V


def _archive_table(model, reps, hmask, slot_h, batch_size):
    """The archive table [R, A * D] of a pool_archives encoder (OMAP) for R behaviour rows (hmask [R, H]; slot_h [R, H]: the rows of `reps` of
    the history news): row r holds the A archives of encode_archives, one after the other; `batch_size` rows per encode_archives call."""
    ue, (R, D) = model.user_encoder, (hmask.shape[0], reps.shape[1])
    table = None
    for s in range(0, R, batch_size):
        e = min(s + batch_size, R)
        arch = ue.encode_archives(reps[slot_h[s:e]], hmask[s:e].contiguous())             # [r, A, D]
        if table is None:
            table = torch.empty((R, arch.shape[1] * D), device=reps.device, dtype=torch.float32)
        table[s:e] = arch.reshape(e - s, -1)
    return table


def _archive_args(model, archives):
    """The archive keywords of ops.topk_scores / ops.pool_ranks for `model` under the caller's `archives` keyword: none for an encoder of one
    vector per row."""
    ue = model.user_encoder
    return dict(archives=int(ue.OMAP_head_num), scale=float(ue.archive_scale)) if archives and ue.pool_archives else {}


def _pool_inputs(model, corpus, rows, pool, exclude_history, batch_size, dedup_users, archives, *extra):
    """What recommend and rank_in_pool hand to their launch (model in eval mode): the distinct news of the histories, the pool and `extra`
    (further vectors of news indices) are encoded once into `reps` (row i = news used[i], ascending), the user encoder runs once per row of
    `rows` (once per distinct (user, history, mask) row with dedup_users) into `table` (one vector per row; for a pool_archives encoder its A
    archives per row, [rows, A * D], from one encode_archives call per batch of distinct rows); valid marks the pool's rows of reps; exclude holds
    the table rows of the live history slots with -1 in the dead ones (None unless exclude_history).  back: the user row of every entry of
    `rows` (None: its own position); slot_x: the rows of reps of each of `extra`."""
    t = corpus.t
    users, hist, hmask = t['beh_user'][rows], t['beh_history'][rows].long(), t['beh_history_mask'][rows] != 0
    back = None
    if dedup_users:
        users, hist, hmask, back = _distinct_rows(users, hist, hmask)
    used, reps, (slot_h, slot_p, *slot_x) = _news_table(model, corpus, hist, pool, *extra)
    if archives and model.user_encoder.pool_archives:
        table = _archive_table(model, reps, hmask, slot_h, batch_size)
    else:
        table = _user_table(model, corpus, reps, users, hist, hmask, slot_h, None, batch_size)
    valid = torch.zeros(used.numel(), device=corpus.device, dtype=torch.uint8)
    valid[slot_p] = 1
    exclude = torch.where(hmask, slot_h, -1).to(torch.int32).contiguous() if exclude_history else None      # a dead slot is -1
    return table, reps, used, valid, exclude, back, slot_x


@torch.no_grad()
def recommend(model, corpus, K, rows=None, pool=None, exclude_history=True, batch_size=256, dedup_users=True, check=True, archives=False):
    """(news int64 [R, K], scores float32 [R, K]) on the device: for each of the behaviour rows `rows` of `corpus` (default: all) the K news of
    `pool` (news indices; default: every news of the corpus but PAD news 0) with the largest click scores, best first, equal scores by
    ascending position in the sorted table of distinct news (= ascending news index); -1 / -inf where the pool ran out.  exclude_history: a
    news in a live history slot of the row is not recommended to it.  The distinct news are encoded once, the user encoder runs once per
    row (once per distinct (user, history, mask) row with dedup_users), and ONE nnr_topk_scores launch ranks the pool.  1 <= K <= 64.
    archives=True: a pool_archives encoder (OMAP) is served too -- a row is its A archives and the launch is nnr_topk_archive_scores: the
    click score as the softmax-weighted sum over the archives' inner products.  Without it such a model is refused as
    every candidate-aware one, which is what recommend did before the archive form existed; other models are served the same either way.
    Refused (NnrHipError naming the reason, recommend_refusal) for news encoders whose representations cannot be cached, user encoders
    whose vector depends on the candidate other than through such archives, and any click predictor but dot_product."""
    why = recommend_refusal(model, archives)
    if why is not None:
        raise L.NnrHipError(why)
    rows, pool, _ = _pool_rows('recommend', corpus, rows, pool)
    with eval_mode(model):
        table, reps, used, valid, exclude, back, _ = _pool_inputs(model, corpus, rows, pool, exclude_history, batch_size, dedup_users, archives)
        idx, scores = ops.topk_scores(table, reps, K, valid=valid, exclude=exclude, check=check, **_archive_args(model, archives))
        news = torch.where(idx >= 0, used[idx.long().clamp_min(0)], -1)
        if back is not None:
            news, scores = news[back], scores[back]
    LAST_STATS.update(mode='recommend', rows=int(rows.numel()), user_rows=int(table.shape[0]), encoder_rows=int(used.numel()),
                      pool=int(pool.numel()), K=int(K), archives=_archive_args(model, archives).get('archives', 1))
    return news, scores


# ------------------------------------------------------------------------------------------------ full-pool ranks
# recommend returns lists; rank_in_pool says how good they are: the place of the news a row actually clicked among the eligible news of the
# pool, which is the number of entries recommend's list would hold before it -- counted by nnr_pool_ranks without the list, for any depth.
def clicked_targets(corpus, labels):
    """(rows, targets) for rank_in_pool: the samples of a dev corpus with label 1 (sample i reads behaviour row i) and their candidates, int64
    device vectors in sample order."""
    lab = torch.as_tensor(np.asarray(labels) if not torch.is_tensor(labels) else labels).to(corpus.device).reshape(-1)
    if lab.numel() != corpus.num:
        raise ValueError('clicked_targets: %d labels for %d samples' % (lab.numel(), corpus.num))
    rows = torch.nonzero(lab == 1).reshape(-1)
    return rows, corpus.samples[rows, 0].long()


def pool_rank_metrics(ahead, pool_size, ks=(5, 10)):
    """The full-ranking metrics of `ahead` / `pool_size` (integer device vectors of one length) as Python numbers, float64 on the device, one
    read-back.  Over the counted targets (ahead >= 0): hr@k = mean[ahead < k], ndcg@k = mean[ahead < k ? 1 / log2(ahead + 2) : 0],
    mrr = mean[1 / (ahead + 1)]; percentile = mean[1 - ahead / (pool_size - 1)] over the counted ones with pool_size > 1; counted and skipped
    are integers.  A mean over nothing is NaN."""
    counted = ahead >= 0
    a = ahead.clamp_min(0).to(torch.float64)
    zero = torch.zeros((), device=ahead.device, dtype=torch.float64)
    n = counted.sum().to(torch.float64)
    names, vals = ['counted', 'skipped'], [n, (~counted).sum().to(torch.float64)]
    for k in ks:
        hit = counted & (ahead < k)
        names += ['hr@%d' % k, 'ndcg@%d' % k]
        vals += [hit.sum().to(torch.float64) / n, torch.where(hit, 1.0 / torch.log2(a + 2.0), zero).sum() / n]
    ranked = counted & (pool_size > 1)
    names += ['mrr', 'percentile']
    vals += [torch.where(counted, 1.0 / (a + 1.0), zero).sum() / n,
             torch.where(ranked, 1.0 - a / (pool_size.to(torch.float64) - 1.0).clamp_min(1.0), zero).sum() / ranked.sum().to(torch.float64)]
    out = dict(zip(names, torch.stack(vals).tolist()))
    out['counted'], out['skipped'] = int(out['counted']), int(out['skipped'])
    return out


@torch.no_grad()
def rank_in_pool(model, corpus, rows, targets, pool=None, exclude_history=True, ks=(5, 10), batch_size=256, dedup_users=True, check=True,
                 archives=False):
    """(ahead int32 [R], pool_size int32 [R], metrics) for the behaviour rows `rows` of `corpus` (repeats allowed) and one target news index per
    entry of `rows`: ahead[i] = the number of eligible news of `pool` that the model ranks before targets[i] for rows[i] -- the number of
    entries recommend's list would hold before it, with recommend's pool, history exclusion and tie order --, -1 when the target is itself
    not eligible for the row (outside the pool, or in a live history slot with exclude_history); pool_size[i] = the row's eligible news.
    Both on the device, in the order of `rows`.  metrics: pool_rank_metrics over the counted targets, Python numbers.  Other targets of the
    same row count as ahead of a target when they precede it.  The path is recommend's (news encoded once, the user encoder once per
    distinct row), followed by ONE nnr_pool_ranks launch (nnr_pool_archive_ranks for OMAP with archives=True, as in recommend); refused for
    the models recommend refuses, with recommend_refusal's words."""
    why = recommend_refusal(model, archives)
    if why is not None:
        raise L.NnrHipError(why)
    rows, pool, V = _pool_rows('rank_in_pool', corpus, rows, pool)
    dev = corpus.device
    targets = _index_list('targets', targets, V, dev, 'rank_in_pool')
    if targets.numel() != rows.numel():
        raise ValueError('rank_in_pool: %d targets for %d rows (one target per entry of rows)' % (targets.numel(), rows.numel()))
    with eval_mode(model):
        table, reps, used, valid, exclude, back, (slot_t,) = _pool_inputs(model, corpus, rows, pool, exclude_history, batch_size, dedup_users, archives, targets)
        urow = back if back is not None else torch.arange(rows.numel(), device=dev)
        order = torch.argsort(urow, stable=True)                                # the targets grouped by user row
        t_off = torch.zeros(table.shape[0] + 1, device=dev, dtype=torch.int64)
        t_off[1:] = torch.cumsum(torch.bincount(urow, minlength=table.shape[0]), dim=0)
        a, _, psz = ops.pool_ranks(table, reps, t_off.to(torch.int32), slot_t[order].to(torch.int32).contiguous(), valid=valid, exclude=exclude,
                                   check=check, **_archive_args(model, archives))
        ahead = torch.empty_like(a)
        ahead[order] = a                                                        # back into the order of `rows`
        pool_size = psz[urow]
        metrics = pool_rank_metrics(ahead, pool_size, ks)
    LAST_STATS.update(mode='rank_in_pool', rows=int(rows.numel()), user_rows=int(table.shape[0]), encoder_rows=int(used.numel()),
                      pool=int(pool.numel()), targets=int(targets.numel()), archives=_archive_args(model, archives).get('archives', 1))
    return ahead, pool_size, metrics


# ------------------------------------------------------------------------------------------------ de-duplicated evaluation
# CNE and CNE_wo_CA gate the title at title-rank r of an encoder call with the content memory (final cell state) at content-rank r of the
# same call, and the other way round: a representation depends on its batch-mates, so nothing above applies.  But only through TWO of them:
# with the 'stable' tie order  rep(i) = f(news_i, news_pc(i), news_pt(i)),  pc(i) / pt(i) = the sequence whose content / title memory gates
# title / content i, and both follow from the per-news lengths and the composition of the call.  So the pairing of every call of the
# reference's batches is planned on the device (nnr_cne_pair_triples), the memories are computed once per distinct news of the split, and a
# full representation once per distinct (news, partner, partner) triple of a window of batches -- with the scores of the reference's batches.
def dedup_refusal(model):
    """None when compute_scores_dedup can score `model`, else the reason it cannot."""
    ne, ue = model.news_encoder, model.user_encoder
    name = type(ne).__name__
    if not ne.cne_gate or ne.batch_independent:
        return ('de-duplicated evaluation is for the news encoders that pair the sequences of a call by sorted rank (CNE, CNE_wo_CA): %s does '
                'not (cne_gate) -- %s' % (name, 'its representations are cached per news instead (compute_scores_cached)'
                                          if ne.batch_independent else 'its dependence on the call is not a pairing'))
    if ne.tie_order != 'stable':
        return ('de-duplicated evaluation plans the pairing on the device in the stable order of equal lengths: %s has tie_order=%r, whose '
                'order is the host sort\'s, call by call' % (name, ne.tie_order))
    if not hasattr(ue, 'encode_user'):
        return 'de-duplicated evaluation hands gathered representations to the user encoder: %s has no encode_user' % type(ue).__name__
    return None


def dedup_supported(model):
    return dedup_refusal(model) is None


def news_lengths(corpus):
    """(tlen, clen) int32 [news]: the ones of every news' title / abstract mask with position 0 forced to 1 (newsEncoders.py:108-109)."""
    out = []
    for k in ('news_title_mask', 'news_abstract_mask'):
        m = corpus.t[k] != 0
        out.append((m.sum(dim=1) + (~m[:, 0]).long()).to(torch.int32).contiguous())
    return tuple(out)


def _news_fields(t, sel):
    """The encoder inputs of the news `sel` as ONE call of len(sel) sequences: [1, n, ...] copies (the encoder fixes its masks in place)."""
    f = lambda k: t[k][sel].unsqueeze(0).contiguous()
    return (f('news_title_text'), f('news_title_mask'), f('news_abstract_text'), f('news_abstract_mask'), f('news_category'),
            f('news_subCategory'))


@torch.no_grad()
def compute_scores_dedup(model, corpus, batch_size, window=64, chunk=4096):
    """The scores of compute_scores(model, corpus, batch_size, cache=False) -- the reference's batches of `batch_size` consecutive samples,
    its pairing inside every encoder call -- with every distinct news' memories computed once per split and every distinct
    (news, partner, partner) triple encoded once per window of `window` batches, in calls of up to `chunk` sequences.  Exact up to the
    regrouping of the products' rows.  Refused (NnrHipError naming the reason, dedup_refusal) for every model but CNE / CNE_wo_CA with the
    stable tie order and a user encoder that has encode_user."""
    from . import news_encoders as NE
    from .model import _DotProductFn
    why = dedup_refusal(model)
    if why is not None:
        raise L.NnrHipError(why)
    if window < 1:
        raise ValueError('compute_scores_dedup: window=%d' % window)
    if corpus.t['news_title_mask'].shape[0] ** 3 >= 2 ** 63:
        raise L.NnrHipError('compute_scores_dedup packs a triple of news ids into one int64 word: %d news are too many' % corpus.t['news_title_mask'].shape[0])
    ne = model.news_encoder
    t, dev = corpus.t, corpus.device
    hist, cand = t['beh_history'].contiguous(), corpus.samples[:, 0].contiguous()
    n, H = hist.shape
    V = t['news_title_mask'].shape[0]
    tlen, clen = news_lengths(corpus)
    with eval_mode(model):
        # the memories (final cell states of both streams) of every distinct news: they depend on the news alone
        used = torch.unique(torch.cat([hist.reshape(-1), cand]).long())
        U, H2 = used.numel(), 2 * ne.hidden_dim
        row_of = torch.full((V,), -1, device=dev, dtype=torch.int32)
        row_of[used] = torch.arange(U, device=dev, dtype=torch.int32)
        mem_t, mem_c = (torch.empty((U, H2), device=dev, dtype=torch.float32) for _ in range(2))
        for s in range(0, U, chunk):
            sel = used[s:s + chunk]
            sv = NE._cne_fwd_pre_and_lstm(ne, *_news_fields(t, sel), None)
            for mem, st in zip((mem_t, mem_c), sv['streams']):
                mem[s:s + sel.numel()] = st['cn'][st['plan'].rank.long()]             # cn is stored by sorted rank
        scores = torch.zeros(n, device=dev, dtype=torch.float32)
        triples = windows = 0
        span = window * batch_size
        for w0 in range(0, n, span):
            cnt = min(span, n - w0)
            w = slice(w0, w0 + cnt)
            pc_h, pt_h, pc_c, pt_c = ops.cne_pair_triples(hist, cand, tlen, clen, batch_size, w0, cnt, check=w0 == 0)
            own = torch.cat([hist[w].reshape(-1), cand[w]]).long()
            key = torch.stack([own, torch.cat([pc_h.reshape(-1), pc_c]).long(), torch.cat([pt_h.reshape(-1), pt_c]).long()], dim=1)
            word, inv = torch.unique((key[:, 0] * V + key[:, 1]) * V + key[:, 2], return_inverse=True)      # one sortable word per triple
            trip = torch.stack([word // (V * V), word // V % V, word % V], dim=1)
            T = trip.shape[0]
            reps = torch.empty((T, ne.news_embedding_dim), device=dev, dtype=torch.float32)
            for s in range(0, T, chunk):
                part = trip[s:s + chunk]
                sv = NE._cne_fwd_pre_and_lstm(ne, *_news_fields(t, part[:, 0]), None)
                pt_, pc_ = sv['streams'][0]['plan'], sv['streams'][1]['plan']
                # the title at sorted position s is sequence order_t[s]: gated by the content memory of its triple's second news
                sv['cn_override'] = ((mem_c, row_of[part[:, 1]][pt_.order.long()].contiguous()),
                                     (mem_t, row_of[part[:, 2]][pc_.order.long()].contiguous()))
                rep, _ = NE._cne_fwd_post(ne, sv, False)
                reps[s:s + part.shape[0]] = rep.view(part.shape[0], -1)
            slot_h, slot_c = _split_like(inv, (hist[w], cand[w].view(-1, 1)))
            # users and scores of the window's samples, in the reference's batches (a window starts on a batch boundary)
            for s, e, user, c in _encoded_users(model, corpus, reps, t['beh_user'][w], hist[w], t['beh_history_mask'][w], slot_h, slot_c, batch_size):
                scores[w0 + s:w0 + e] = _DotProductFn.apply(user, c).squeeze(dim=1)
            triples += T
            windows += 1
    LAST_STATS.update(mode='dedup', triples=int(triples), distinct_news=int(U), per_sample_rows=int(n * (H + 1)), windows=int(windows))
    return scores


def rank_metrics(scores, labels, sizes):
    """scores float32 [n], labels uint8/bool [n], sizes: candidates per impression (contiguous, file order).
    Returns (ranks int32 [n], per_impression float64 [n_imp, 4], means float64 [4]) -- all device tensors."""
    dev = scores.device
    sizes = torch.as_tensor(np.asarray(sizes), dtype=torch.int64)
    offsets = torch.zeros(sizes.numel() + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(sizes, 0)
    assert int(offsets[-1]) == scores.numel() == labels.numel()
    offsets = offsets.to(dev)
    lab = labels.to(device=dev, dtype=torch.uint8).contiguous()
    ranks = torch.empty(scores.numel(), device=dev, dtype=torch.int32)
    per = torch.empty((sizes.numel(), 4), device=dev, dtype=torch.float64)
    L.check(L.lib().nnr_rank_metrics(_p(scores.contiguous()), _p(lab), _p(offsets), sizes.numel(), _p(ranks), _p(per), _s()), 'nnr_rank_metrics')
    return ranks, per, per.mean(dim=0)


def evaluate(model, corpus, labels, sizes, batch_size, listwise=False, dedup=False):
    """compute_scores + scoring: -> (auc, mrr, ndcg5, ndcg10) as Python floats, plus the ranks (for the result file).  listwise=True scores
    each impression as a list (compute_scores_listwise) when the model allows it (listwise_supported), and as without the keyword otherwise.
    dedup=True scores the rank-pairing CNE encoders triple by triple (compute_scores_dedup) when the model allows it (dedup_supported); any
    other model, a news_reps_cacheable one included, keeps the path it has without the keyword."""
    if listwise and listwise_supported(model):
        scores = compute_scores_listwise(model, corpus, sizes, batch_size)
    elif dedup and dedup_supported(model):
        scores = compute_scores_dedup(model, corpus, batch_size)
    else:
        scores = compute_scores(model, corpus, batch_size)
    ranks, _, means = rank_metrics(scores, torch.as_tensor(np.asarray(labels)), sizes)
    return tuple(float(v) for v in means.cpu()), ranks


def write_result_file(path, ranks, sizes):
    """The submission format of util.py:53-60: line i = '<i> [rank of candidate 0, rank of candidate 1, ...]'."""
    r = ranks.cpu().numpy().tolist()
    o = 0
    with open(path, 'w', encoding='utf-8') as f:
        for i, n in enumerate(sizes):
            f.write(('' if i == 0 else '\n') + str(i + 1) + ' ' + str(r[o:o + n]).replace(' ', ''))
            o += n
