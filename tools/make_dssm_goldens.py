#!/usr/bin/env python3
"""Generate tests/golden/dssm_*.npz by running the REFERENCE's own DSSM_model.DSSM on the CPU.

Runs only in the build container (needs /root/reference); nothing of the reference travels: the fixtures hold inputs, expected outputs
(arrays) and settings only.  Accommodations, none of which touch the arithmetic:
  * DSSM_util.Config() asserts a GPU and reads the dataset's pickles -> a SimpleNamespace with the attributes DSSM_model reads;
  * the six nn.Dropout calls of a forward pass are observed through a forward hook on the model's one Dropout module: the keep-mask of a
    call is (output != 0) | (input == 0) -- where the input is zero (a zero tf-idf weight) the mask cannot matter;
  * the training step is DSSM_main.py:62-69 (loss, zero_grad, backward, clip_grad_norm_, Adam.step), restated here in five lines, since
    DSSM_main.Trainer cannot be built without the dataset;
  * the tiny split's metrics come from the reference's `scoring` (general_recommendation_methods/evaluate.py) fed the rank lists that
    DSSM_util.compute_scores writes (scores sorted descending per impression), through in-memory files.
Large arrays of the wide case are kept as tests/dssm_ref.py:sample keeps them; its parameters come from tests/golden_weights.make_state.

Usage:  python tools/make_dssm_goldens.py"""
import io
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference/general_recommendation_methods'
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from dssm_ref import PARAMS, SITES, sample          # noqa: E402
from golden_weights import make_state              # noqa: E402
from nnr_amd.synth import tfidf_rows               # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
STEPS = 3


def tables(rng, U, M, Lu, Ln, V):
    """User / news term-vector tables without an empty row (an empty news row is excluded: the reference's dataset never yields one for a
    news that has any term), sharing ids across rows and across the two sides (V is small against the rows' lengths)."""
    ui, uw = tfidf_rows(rng, U + 1, Lu, V)
    ni, nw = tfidf_rows(rng, M + 1, Ln, V)
    ui, uw = ui[(uw != 0).any(axis=1)][:U], uw[(uw != 0).any(axis=1)][:U]
    ni, nw = ni[(nw != 0).any(axis=1)][:M], nw[(nw != 0).any(axis=1)][:M]
    assert ui.shape[0] == U and ni.shape[0] == M
    assert np.intersect1d(ui[uw != 0], ni[nw != 0]).size > 0
    return ui, uw, ni, nw


def seq_len(w):
    n = (w != 0).sum(axis=-1).astype(np.float32)
    return np.where(n == 0, np.float32(1e12), n)         # DSSM_util.py:22


def record_masks(model):
    calls = []

    def hook(_module, inp, out):
        calls.append(((out != 0) | (inp[0] == 0)).detach().clone())
    return calls, model.dropout.register_forward_hook(hook)


def make(tag, B, N, Lu, Ln, V, H, Fd, p, seed, wide=False):
    import DSSM_model
    from evaluate import scoring
    rng = np.random.default_rng(seed)
    U, M = B + 1, B * N - 2                             # fewer news than slots: candidates repeat across samples
    ui, uw, ni, nw = tables(rng, U, M, Lu, Ln, V)
    user_sel = rng.permutation(U)[:B].astype(np.int32)
    news_sel = rng.integers(0, M, (B, N)).astype(np.int32)
    cfg = SimpleNamespace(vocabulary_size=V, DSSM_hidden_dim=H, DSSM_feature_dim=Fd, dropout_rate=p)
    torch.manual_seed(seed)
    model = DSSM_model.DSSM(cfg)
    model.initialize()
    meta = dict(vocabulary_size=V, DSSM_hidden_dim=H, DSSM_feature_dim=Fd, dropout_rate=p, user_word_num=Lu, news_word_num=Ln,
                negative_sample_num=N - 1, batch_size=B, lr=1e-3, weight_decay=0.0, gradient_clip_norm=4.0 if not wide else 0.5, seed=seed,
                adam_steps=STEPS, shapes={k: list(v.shape) for k, v in model.state_dict().items()})
    out = {}
    if wide:
        meta.update(weight_seed=seed, weight_gain=1.0)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in make_state(meta['shapes'], seed, 1.0).items()}, strict=True)
    else:
        for k, v in model.state_dict().items():
            out['param/' + k] = v.numpy().copy()
    assert tuple(model.state_dict()) == PARAMS
    batch = (ui[user_sel].astype(np.int64), uw[user_sel], seq_len(uw[user_sel]), ni[news_sel].astype(np.int64), nw[news_sel], seq_len(nw[news_sel]))
    for k, v in zip(('user_indices', 'user_weights', 'user_seq_len', 'news_indices', 'news_weights', 'news_seq_len'), batch):
        out['in/' + k] = v
    out.update({'corpus/user_ids': ui, 'corpus/user_w': uw, 'corpus/news_ids': ni, 'corpus/news_w': nw, 'in/user_sel': user_sel, 'in/news_sel': news_sel})
    tb = [torch.from_numpy(np.ascontiguousarray(v)) for v in batch]

    # the tiny split, eval mode, the per-sample form of DSSM_util.compute_scores
    sizes = np.array([3, 2, 4, 3], dtype=np.int64)
    s_user = np.repeat(rng.integers(0, U, sizes.size), sizes).astype(np.int32)
    s_news = np.concatenate([rng.permutation(M)[:n] for n in sizes]).astype(np.int32)
    labels = np.concatenate([np.roll(np.arange(n) == 0, int(rng.integers(n))) for n in sizes]).astype(np.uint8)
    model.eval()
    with torch.no_grad():
        scores = model(torch.from_numpy(ui[s_user].astype(np.int64)), torch.from_numpy(uw[s_user]), None,
                       torch.from_numpy(ni[s_news].astype(np.int64)).unsqueeze(1), torch.from_numpy(nw[s_news]).unsqueeze(1), None).squeeze(1).numpy()
    truth, result, o = [], [], 0
    for i, n in enumerate(sizes):
        sc = scores[o:o + n]
        assert np.unique(sc).size == n and np.diff(np.sort(sc)).min() > 1e-4, 'tiny-split scores must be free of (near) ties'
        order = sorted(range(n), key=lambda j: sc[j], reverse=True)
        rank = [0] * int(n)
        for pos, j in enumerate(order):
            rank[j] = pos + 1
        truth.append('%d %s' % (i + 1, str(labels[o:o + n].tolist()).replace(' ', '')))
        result.append('%d %s' % (i + 1, str(rank).replace(' ', '')))
        o += n
    metrics = scoring(io.StringIO('\n'.join(truth)), io.StringIO('\n'.join(result)))
    out.update({'eval/sample_user': s_user, 'eval/sample_news': s_news, 'eval/labels': labels, 'eval/sizes': sizes, 'eval/scores': scores,
                'eval/metrics': np.array(metrics, dtype=np.float64)})

    # three training steps (DSSM_main.py:62-69)
    model.train()
    calls, handle = record_masks(model)
    opt = torch.optim.Adam(model.parameters(), lr=meta['lr'], weight_decay=meta['weight_decay'])
    for s in range(STEPS):
        del calls[:]
        logits = model(*tb)
        loss = -torch.log_softmax(logits, dim=1).select(1, 0).mean()
        opt.zero_grad()
        loss.backward()
        assert len(calls) == len(SITES)
        if p > 0:
            for site, k in zip(SITES, calls):
                out['mask%d/%s' % (s, site)] = k.squeeze(1).numpy() if site == 'user_y' else k.numpy()
        out['loss_step%d' % s] = np.float32(loss.item())
        if s == 0:
            out['logits'] = logits.detach().numpy().copy()
            out['loss'] = np.float32(loss.item())
            total = 0.0
            for k, v in model.named_parameters():
                out['grad/' + k] = sample(v.grad.numpy().copy())
                out['gradnorm/' + k] = np.float64(v.grad.double().norm().item())
                total += float(v.grad.double().pow(2).sum())
            out['grad_total_norm'] = np.float64(total ** 0.5)
        if meta['gradient_clip_norm'] > 0:
            torch.nn.utils.clip_grad_norm_(model.parameters(), meta['gradient_clip_norm'])
        opt.step()
    handle.remove()
    for k, v in model.state_dict().items():
        out['param%d/%s' % (STEPS, k)] = sample(v.numpy().copy())
    # (at p = 0.5 and five features a whole row of y is dropped now and then: 0 / 0.  The committed seed is one whose three steps are finite.)
    assert all(np.isfinite(out['loss_step%d' % s]) for s in range(STEPS)), 'seed %d: a step lost a whole feature row to dropout' % seed
    out['meta'] = np.array(json.dumps(meta))
    path = os.path.join(OUT, tag + '.npz')
    np.savez_compressed(path, **out)
    print('%s: %.1f KB, loss %s, metrics %s' % (tag, os.path.getsize(path) / 1024.0, [float(out['loss_step%d' % s]) for s in range(STEPS)], metrics))


if __name__ == '__main__':
    make('dssm_tiny', B=3, N=3, Lu=9, Ln=4, V=37, H=6, Fd=5, p=0.0, seed=11)
    make('dssm_tiny_wide', B=3, N=3, Lu=70, Ln=4, V=211, H=512, Fd=512, p=0.0, seed=12, wide=True)
    make('dssm_drop_tiny', B=3, N=3, Lu=9, Ln=4, V=37, H=6, Fd=5, p=0.5, seed=21)
