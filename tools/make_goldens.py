#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REFERENCE's own model.py on CPU.

Runs only in the build container (needs /root/reference); nothing of the reference travels:
the fixtures hold inputs and expected outputs (arrays) only.  Accommodations, none of which
touch the arithmetic:
  * torch_scatter (third-party, absent) -> tools/ref_shims/torch_scatter.py (pure torch composite);
  * config.Config() cannot be built without a GPU/dataset -> a SimpleNamespace with the same attributes;
  * NewsEncoder.__init__ unpickles the word table from CWD -> a synthetic table is written to a temp CWD;
  * the loss is the trainer's (trainer.py:109-114): the encoders' `auxiliary_loss.mean()` is added when it is not None.  It is None for
    every encoder pair but those with the OMAP user encoder, whose fixtures also store the term as `auxiliary_loss`;
  * OMAP.initialize() calls `self.J_k.cuda()` and drops the result (userEncoders.py:348-349), which raises without a GPU: the `omap`
    cases build the model with torch.Tensor.cuda patched to the identity (as tools/make_eval_goldens.py does);
  * `OMAP_head_num` / `HiFi_Ark_regularizer_coefficient` (config.py:74-75) enter the attribute bag through tiny_cfg / full_cfg keywords.

Usage:  python tools/make_goldens.py            (rewrites every fixture)
        python tools/make_goldens.py catt       (the CATT user encoder and the candidate-attention layers)
        python tools/make_goldens.py omap       (the OMAP user encoder)
        python tools/make_goldens.py npa        (the PNE news encoder and the PUE user encoder on the user-id embedding path)
        python tools/make_goldens.py bow        (the DAE and Inception bag-of-words news encoders)
        python tools/make_goldens.py kcnn       (the KCNN news encoder of DKN, with entity ids written into the batches)
        python tools/make_goldens.py fim        (the HDC news encoder, the FIM user encoder and the FIM click head)
        python tools/make_goldens.py gru        (the GRU user encoder of DAE-GRU)
        python tools/make_goldens.py naml       (the single-view NAML news encoders NAML_Title / NAML_Content)
        python tools/make_goldens.py sue_ablation   (the user-encoder ablations SUE_wo_GCN / SUE_wo_HCA)
        python tools/make_goldens.py cne_ablation   (the news-encoder ablations CNE_Title / CNE_Content / CNE_wo_CS / CNE_wo_CA)
"""
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference'
sys.path.insert(0, os.path.join(ROOT, 'tools', 'ref_shims'))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from golden_weights import make_state          # noqa: E402
from nnr_amd.synth import SynthSpec, SynthCorpus, BATCH_FIELDS, to_torch   # noqa: E402
from oracle.nnr_oracle import default_config   # noqa: E402  (attribute bag only; no oracle arithmetic used here)

OUT = os.path.join(ROOT, 'tests', 'golden')


def build_reference_model(cfg, word_table):
    import model as ref_model                   # /root/reference/model.py
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        name = 'word_embedding-%d-%d-%s-%d-%d-%s.pkl' % (cfg.word_threshold, cfg.word_embedding_dim, cfg.tokenizer,
                                                         cfg.max_title_length, cfg.max_abstract_length, cfg.dataset)
        with open(name, 'wb') as f:
            pickle.dump(torch.from_numpy(word_table), f)
        if cfg.news_encoder == 'KCNN':          # newsEncoders.py:212-215 unpickles both knowledge tables too (make_state overwrites them)
            rngk = np.random.default_rng(cfg.entity_size)
            for kind, dim in (('entity', cfg.entity_embedding_dim), ('context', cfg.context_embedding_dim)):
                with open('%s_embedding-%s.pkl' % (kind, cfg.dataset), 'wb') as f:
                    pickle.dump(torch.from_numpy((0.1 * rngk.standard_normal((cfg.entity_size, dim))).astype(np.float32)), f)
        try:
            m = ref_model.Model(cfg)
        finally:
            os.chdir(cwd)
    m.initialize()
    if cfg.user_encoder == 'GRU':               # userEncoders.py:310,327 allocate the empty users' zero rows on self.device ('cuda')
        m.user_encoder.device = torch.device('cpu')
    return m


class stable_sort_patch:
    """Version-skew accommodation for the *_stable fixtures: the reference pins torch 1.12.1, whose CPU
    torch.sort is a stable sort; this container's torch 2.10 uses an unstable std::sort for n > 16.  The
    tie order is observable (newsEncoders.py:112-115,128-129 pair the two streams by sorted rank), so the
    *_stable fixtures run the reference with torch.sort forced stable, i.e. as under its pinned torch.
    The unsuffixed fixtures run the reference untouched."""

    def __enter__(self):
        self.orig = torch.sort
        orig = self.orig

        def sort(input, dim=-1, descending=False, stable=False, **kw):
            return orig(input, dim=dim, descending=descending, stable=True, **kw)
        torch.sort = sort

    def __exit__(self, *a):
        torch.sort = self.orig


class record_dropout:
    """Dropout-ON fixtures (`python tools/make_goldens.py dropout`): the reference runs in train mode with its dropout modules
    active; every call of torch.nn.functional.dropout (nn.Dropout.forward and the F.dropout of userEncoders.py:171 both end
    there) draws its keep-mask from a seeded numpy generator instead of torch's Philox stream, applies the SAME arithmetic
    (x * keep / (1 - p), in place when the reference asks for in place) and records (p, mask) in call order.  The fixture
    stores the masks; the oracle replays them at its own dropout sites (oracle.forced_dropout), which pins WHERE each site sits,
    its p (rate, rate / 2 between GCN layers, 0.5 at userEncoders.py:171), its shape and its scale to the reference itself."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.calls = []

    def __enter__(self):
        import torch.nn.functional as F
        self.F, self.orig = F, F.dropout

        def dropout(input, p=0.5, training=True, inplace=False):
            if not training or p == 0.0:
                return input
            keep = self.rng.random(tuple(input.shape)) >= p
            self.calls.append((float(p), keep))
            m = torch.from_numpy(keep.astype(np.float32)) * (1.0 / (1.0 - p))
            return input.mul_(m) if inplace else input * m
        F.dropout = dropout
        return self

    def __exit__(self, *a):
        self.F.dropout = self.orig


def run_case(tag, cfg, spec, batch_size, seed, mode, gain=None, full_arrays=True, adam_steps=3, dropout_seed=None, _rec_drop=None, user_ids=None, f64_step=False, entity_seed=None,
             batch_hook=None, all_masks=False, rep_grads=False):
    """mode: 'train' (dropout_rate must be 0 unless dropout_seed is given) or 'eval' (for MHSA-user's hard-wired F.dropout).
    user_ids: the batch's user_ID (int64 [batch_size]) instead of the synthetic corpus's arange -- the personalised encoders read it.
    entity_seed: write entity ids into the batch's title_entity fields (tests/kcnn_ref.py:fill_entities; the synthetic corpus leaves them zero).
    batch_hook: edits the batch's arrays in place before anything reads them.  all_masks: store the mutated copies of all four text masks
    (`mutated_{news,user}_{title,content}_mask`).  rep_grads (with f64_step): store the float64 run's gradients of the loss with respect to
    the two news-encoder outputs (`f64/dcand_rep`, `f64/dhist_rep`)."""
    if dropout_seed is not None:
        assert adam_steps == 1 and mode == 'train'
        with record_dropout(dropout_seed) as rec_drop:
            return run_case(tag, cfg, spec, batch_size, seed, mode, gain, full_arrays, adam_steps, None, _rec_drop=rec_drop, user_ids=user_ids)
    torch.manual_seed(seed)
    corpus = SynthCorpus(spec)
    batch = corpus.batch(batch_size, np.random.default_rng(seed + 100))
    if user_ids is not None:
        batch['user_ID'] = np.asarray(user_ids, dtype=np.int64).reshape(batch_size)
    if entity_seed is not None:
        from kcnn_ref import fill_entities
        fill_entities(batch, cfg.entity_size, entity_seed)
    if batch_hook is not None:
        batch_hook(batch)
    rngw = np.random.default_rng(seed + 7)
    table = (rngw.standard_normal((cfg.vocabulary_size, cfg.word_embedding_dim)) * 0.3).astype(np.float32)
    table[0] = 0
    m = build_reference_model(cfg, table)
    shapes = {k: tuple(v.shape) for k, v in m.named_parameters()}
    if gain is not None:                        # deterministic, regenerable weights
        st = make_state(shapes, seed, gain)
        with torch.no_grad():
            for k, p in m.named_parameters():
                p.copy_(torch.from_numpy(st[k]))
    m.train() if mode == 'train' else m.eval()
    params0 = {k: p.detach().clone().numpy() for k, p in m.named_parameters()}

    rec = {}
    if cfg.news_encoder == 'HDC':               # the representation is the pair (d0, dL); the raw Conv3d outputs (elu runs in place on them)
        m.news_encoder.register_forward_hook(lambda mod, i, o: rec.setdefault('reps', []).append(tuple(t.detach().clone().numpy() for t in o)))
        for name in ('conv_3D_a', 'conv_3D_b'):
            getattr(m.user_encoder, name).register_forward_hook(lambda mod, i, o, name=name: (rec.setdefault(name, o.detach().clone().numpy()), None)[1])
    else:
        m.news_encoder.register_forward_hook(lambda mod, i, o: rec.setdefault('reps', []).append(o.detach().clone().numpy()))
    m.user_encoder.register_forward_hook(lambda mod, i, o: rec.__setitem__('user_rep', o.detach().clone().numpy()))
    if cfg.news_encoder == 'PNE':               # the conv stage's output of both encoder calls, as [titles, L, C] (dropout_ is the identity at p = 0)
        m.news_encoder.conv.register_forward_hook(lambda mod, i, o: rec.setdefault('conv', []).append(o.detach().permute(0, 2, 1).clone().numpy()))

    if cfg.news_encoder == 'DAE':               # the reconstruction term of EACH encoder call (the attribute keeps the last call's only)
        m.news_encoder.register_forward_hook(lambda mod, i, o: rec.setdefault('aux', []).append(float(mod.auxiliary_loss.detach().mean())))

    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=cfg.lr, weight_decay=cfg.weight_decay)
    out = {}
    for step in range(adam_steps):
        inp = to_torch(batch)                   # fresh copies: the model mutates masks in place
        logits = m(*inp)
        loss = (-torch.log_softmax(logits, dim=1).select(dim=1, index=0)).mean()   # trainer.py:64-66
        aux = [e.auxiliary_loss.mean() for e in (m.news_encoder, m.user_encoder) if e.auxiliary_loss is not None]   # trainer.py:109-114
        for a in aux:
            loss = loss + a
        if aux and step == 0:
            out['auxiliary_loss'] = np.float32(float(sum(a.detach() for a in aux)))
        opt.zero_grad()
        loss.backward()
        if step == 0:
            out['logits'] = logits.detach().numpy().copy()
            out['loss'] = np.float32(float(loss))
            if cfg.news_encoder == 'HDC':           # (at full dimensions the two pairs are 10 MB: the tiny fixtures alone hold them)
                for key, rep in (('cand_rep', rec['reps'][0]), ('hist_rep', rec['reps'][1])) if full_arrays else ():
                    out[key + '/d0'], out[key + '/dL'] = rep
            else:
                out['cand_rep'] = rec['reps'][0]
                out['hist_rep'] = rec['reps'][1]
            out['user_rep'] = rec['user_rep']
            if 'aux' in rec:
                out['dae/aux_cand'], out['dae/aux_hist'] = np.float32(rec['aux'][0]), np.float32(rec['aux'][1])
            if 'conv' in rec:
                out['pne/c_cand'] = rec['conv'][0]
                if full_arrays:                 # (the history call's is 0.6 MB compressed at full dimensions: the candidate call's alone there)
                    out['pne/c_hist'] = rec['conv'][1]
            grads = {k: p.grad.detach().clone().numpy() for k, p in m.named_parameters()}
            out['mutated_news_title_mask'] = inp[16].numpy().copy()
            out['mutated_user_history_category_mask'] = inp[11].numpy().copy()
            if all_masks:
                for key, idx in (('news_title', 16), ('news_content', 19), ('user_title', 4), ('user_content', 7)):
                    out['mutated_%s_mask' % key] = inp[idx].numpy().copy()
        total_norm = torch.nn.utils.clip_grad_norm_(m.parameters(), cfg.gradient_clip_norm)
        if step == 0:
            out['grad_total_norm'] = np.float32(float(total_norm))
        opt.step()
        out['loss_step%d' % step] = np.float32(float(loss))
        if step in (0, adam_steps - 1):
            for k, p in m.named_parameters():
                a = p.detach().numpy()
                out['param%d/%s' % (step + 1, k)] = a.copy() if full_arrays else a.reshape(-1)[:64].copy()
    for k, g in grads.items():
        out['gradnorm/' + k] = np.float32(np.linalg.norm(g.astype(np.float64)))
        out['grad/' + k] = g if full_arrays else g.reshape(-1)[:64].copy()
    for k in BATCH_FIELDS:
        out['in/' + k] = batch[k]
    if _rec_drop is not None:
        out['drop_p'] = np.array([p for p, _ in _rec_drop.calls], np.float64)
        for i, (_, keep) in enumerate(_rec_drop.calls):
            out['drop_shape/%d' % i] = np.array(keep.shape, np.int64)
            out['drop_bits/%d' % i] = np.packbits(keep.reshape(-1))
    if f64_step:
        # the reference's own classes once more in float64 (same weights, same batch, step 0 only): `f64/...` = what the fp32 results above
        # round.  Done last, so that nothing above changes; tests pin their float64 restatements to these and read the fp32 arrays' own error
        assert gain is not None and _rec_drop is None
        m64 = build_reference_model(cfg, table)
        with torch.no_grad():
            for k, p in m64.named_parameters():
                p.copy_(torch.from_numpy(st[k]))
        m64 = m64.double()
        m64.train() if mode == 'train' else m64.eval()
        rec64 = []
        fim64 = {}
        if cfg.news_encoder == 'HDC':
            m64.news_encoder.register_forward_hook(lambda mod, i, o: rec64.append(tuple(t.detach().clone().numpy() for t in o)))
            for name in ('conv_3D_a', 'conv_3D_b'):
                getattr(m64.user_encoder, name).register_forward_hook(lambda mod, i, o, name=name: (fim64.setdefault(name, o.detach().clone().numpy()), None)[1])
        else:
            m64.news_encoder.register_forward_hook(lambda mod, i, o: rec64.append(o.detach().clone().numpy()))
        drep64 = {}
        if rep_grads:                           # d loss / d (news-encoder output) of the candidate call (0) and of the history call (1)
            calls64 = []
            m64.news_encoder.register_forward_hook(lambda mod, i, o: (calls64.append(0), o.register_hook(
                lambda g, c=len(calls64) - 1: drep64.__setitem__(c, g.detach().clone().numpy())))[0] and None)
        conv64 = []
        if cfg.news_encoder == 'KCNN':          # the raw convolution outputs of both calls as [titles, positions, C]: the argmax margins
            m64.news_encoder.knowledge_cnn.conv.register_forward_hook(lambda mod, i, o: conv64.append(o.detach().squeeze(3).permute(0, 2, 1).clone().numpy()))
        naml64 = {}
        if cfg.news_encoder in ('NAML_Title', 'NAML_Content'):     # the relu pre-activations of both calls (cloned: the category relus run in place)
            stream = 'title' if cfg.news_encoder == 'NAML_Title' else 'content'
            ne64 = m64.news_encoder
            getattr(ne64, stream + '_conv').conv.register_forward_hook(lambda mod, i, o: naml64.setdefault('z', []).append(o.detach().permute(0, 2, 1).clone().numpy()))
            ne64.category_affine.register_forward_hook(lambda mod, i, o: naml64.setdefault('za', []).append(o.detach().clone().numpy()))
            ne64.subCategory_affine.register_forward_hook(lambda mod, i, o: naml64.setdefault('zs', []).append(o.detach().clone().numpy()))
        inp64 = to_torch(batch)
        inp64[10] = inp64[10].double()          # user_history_graph: torch.bmm (layers.py:286) does not promote
        logits64 = m64(*inp64)
        loss64 = (-torch.log_softmax(logits64, dim=1).select(dim=1, index=0)).mean()
        for e in (m64.news_encoder, m64.user_encoder):
            if e.auxiliary_loss is not None:
                loss64 = loss64 + e.auxiliary_loss.mean()
                out['f64/auxiliary_loss'] = np.float64(float(e.auxiliary_loss.detach().mean()))
        loss64.backward()
        out['f64/logits'], out['f64/loss'] = logits64.detach().numpy().copy(), np.float64(float(loss64.detach()))
        if cfg.news_encoder == 'HDC':
            for key, rep in (('f64/cand_rep', rec64[0]), ('f64/hist_rep', rec64[1])):
                out[key + '/d0'], out[key + '/dL'] = rep
            # the raw Conv3d outputs of the float64 run (the pool margins are read from them) and how far the reference's own fp32
            # convolution outputs are from them, relative to each layer's largest absolute output
            out['f64/fim/za'], out['f64/fim/zb'] = fim64['conv_3D_a'], fim64['conv_3D_b']
            out['fim/conv_dev'] = np.float64(max(float(np.abs(rec[k].astype(np.float64) - fim64[k]).max() / np.abs(fim64[k]).max())
                                                 for k in ('conv_3D_a', 'conv_3D_b')))
        else:
            out['f64/cand_rep'], out['f64/hist_rep'] = rec64[0], rec64[1]
        if rep_grads:
            out['f64/dcand_rep'], out['f64/dhist_rep'] = drep64[0], drep64[1]
        if conv64:
            out['f64/kcnn/z_cand'], out['f64/kcnn/z_hist'] = conv64[0], conv64[1]
        for k, v in naml64.items():
            out['f64/naml/%s_cand' % k], out['f64/naml/%s_hist' % k] = v[0].reshape(-1, v[0].shape[-1]), v[1].reshape(-1, v[1].shape[-1])
        for k, p in m64.named_parameters():
            out['f64/grad/' + k] = p.grad.detach().numpy().copy()
    out['word_table'] = table if gain is None else np.zeros(0, np.float32)
    if gain is None:
        for k, v in params0.items():
            out['param0/' + k] = v
    meta = dict(vars(cfg))
    meta.update(tie_order='stable' if tag.endswith('_stable') else 'torch', case=tag, mode=mode, seed=seed, gain=-1.0 if gain is None else gain, batch_size=batch_size,
                full_arrays=full_arrays, adam_steps=adam_steps)
    out['meta_keys'] = np.array(sorted(meta), dtype=object).astype(str)
    out['meta_vals'] = np.array([str(meta[k]) for k in sorted(meta)], dtype=object).astype(str)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, tag + '.npz'), **out)
    print('%-28s logits[0]=%s loss=%.6f |g|=%.4f' % (tag, np.array2string(out['logits'][0], precision=4), out['loss'],
                                                     out['grad_total_norm']))


def tiny_cfg(news, user, **kw):
    return default_config(news_encoder=news, user_encoder=user, dataset='small', vocabulary_size=64, word_embedding_dim=16,
                          hidden_dim=8, attention_dim=8, max_history_num=6, max_title_length=5, max_abstract_length=9,
                          category_num=3, subCategory_num=7, category_embedding_dim=4, subCategory_embedding_dim=4,
                          negative_sample_num=2, head_num=2, head_dim=4, cnn_kernel_num=12, gcn_layer_num=2,
                          dropout_rate=0.0, lr=1e-2, user_num=4, **kw)


def tiny_spec(cfg, seed):
    return SynthSpec(vocabulary_size=cfg.vocabulary_size, category_num=cfg.category_num, subCategory_num=cfg.subCategory_num,
                     max_title_length=cfg.max_title_length, max_abstract_length=cfg.max_abstract_length,
                     max_history_num=cfg.max_history_num, negative_sample_num=cfg.negative_sample_num, news_pool=40,
                     title_len_mean=3.0, content_len_mean=5.0, empty_content_frac=0.2, empty_history_frac=0.2, seed=seed)


def full_cfg(news, user, V, **kw):
    return default_config(news_encoder=news, user_encoder=user, dataset='200k', vocabulary_size=V, dropout_rate=0.0,
                          gcn_layer_num=4, lr=1e-3, **kw)


def full_spec(cfg, seed):
    return SynthSpec(vocabulary_size=cfg.vocabulary_size, news_pool=300, seed=seed)


def extra_cases():
    """Cases added after round 1 (run with `python tools/make_goldens.py extra`; main() still rewrites the round-1 fixtures
    bit for bit): --gcn_layer_norm (layers.py:273-274,287-288) with and without the GCN residual (one Adam step: with LayerNorm and
    lr 1e-2 the fp32 noise of step 1 is amplified past any useful tolerance by step 3), and hidden sizes that are
    other multiples of 16 than the default 200's 13 unit blocks (config.py:62)."""
    with stable_sort_patch():
        cfg = tiny_cfg('CNE', 'SUE', gcn_layer_norm=True)
        run_case('tiny_CNE_SUE_ln_stable', cfg, tiny_spec(cfg, 3), batch_size=4, seed=23, mode='train', gain=2.0, adam_steps=1)
        cfg = tiny_cfg('CNE', 'SUE', gcn_layer_norm=True, no_gcn_residual=True)
        run_case('tiny_CNE_SUE_ln_nores_stable', cfg, tiny_spec(cfg, 4), batch_size=4, seed=29, mode='train', gain=2.0, adam_steps=1)
        for hd in (48, 112):
            cfg = tiny_cfg('CNE', 'SUE')
            cfg.hidden_dim = hd
            run_case('tiny_CNE_SUE_h%d_stable' % hd, cfg, tiny_spec(cfg, 5), batch_size=3, seed=31 + hd, mode='train', gain=1.0 if hd > 64 else 1.5,
                     full_arrays=False)


def dropout_cases():
    """Round 3: the reference in TRAIN mode with dropout ON (masks recorded, see record_dropout)."""
    with stable_sort_patch():
        cfg = tiny_cfg('CNE', 'SUE')
        cfg.dropout_rate, cfg.gcn_layer_num = 0.2, 3          # two inter-layer GCN dropouts (p/2), none after the last layer
        run_case('drop_tiny_CNE_SUE_stable', cfg, tiny_spec(cfg, 6), batch_size=4, seed=41, mode='train', gain=2.0, adam_steps=1, dropout_seed=1)
    cfg = tiny_cfg('MHSA', 'MHSA')
    cfg.dropout_rate = 0.2
    run_case('drop_tiny_MHSA_MHSA', cfg, tiny_spec(cfg, 7), batch_size=3, seed=43, mode='train', gain=2.0, adam_steps=1, dropout_seed=2)
    cfg = tiny_cfg('CNN', 'ATT')
    cfg.dropout_rate = 0.25
    run_case('drop_tiny_CNN_ATT', cfg, tiny_spec(cfg, 8), batch_size=3, seed=47, mode='train', gain=2.0, adam_steps=1, dropout_seed=3)


def layer_cand_attn():
    """layers.CandidateAttention (layers.py:206-232) and layers.MultipleCandidateAttention (:235-262) of the reference on their own: inputs,
    outputs and every gradient of out.square().sum(), with a mask (one all-zero row, one all-one row, two ragged ones) and with mask=None."""
    import layers as ref_layers                 # the reference's layers.py
    rng = np.random.default_rng(53)
    n, Lx, Fd, Qd, A, Nq = 4, 7, 24, 24, 12, 3
    feature = (0.25 * rng.standard_normal((n, Lx, Fd))).astype(np.float32)      # (gradients of O(1): the fixture's own fp32 rounding stays below 1e-6)
    mask = np.array([[0] * 7, [1] * 7, [1, 1, 1, 0, 0, 0, 0], [1, 0, 1, 1, 1, 0, 0]], dtype=np.int64)
    out = {'feature': feature, 'mask': mask}
    for kind, cls, qshape in (('single', ref_layers.CandidateAttention, (n, Qd)), ('multi', ref_layers.MultipleCandidateAttention, (n, Nq, Qd))):
        mod = cls(Fd, Qd, A)
        mod.initialize()
        st = make_state({k: tuple(v.shape) for k, v in mod.named_parameters()}, 59, 1.5)
        with torch.no_grad():
            for k, p in mod.named_parameters():
                p.copy_(torch.from_numpy(st[k]))
                out['%s/param/%s' % (kind, k)] = st[k]
        out[kind + '/param_names'] = np.array(list(mod.state_dict().keys())).astype(str)
        query = (0.5 * rng.standard_normal(qshape)).astype(np.float32)
        out[kind + '/query'] = query
        for mtag, m in (('mask', torch.from_numpy(mask)), ('nomask', None)):
            f, q = torch.from_numpy(feature.copy()).requires_grad_(), torch.from_numpy(query.copy()).requires_grad_()
            mod.zero_grad()
            o = mod(f, q, m)
            o.square().sum().backward()
            pre = '%s/%s/' % (kind, mtag)
            out[pre + 'out'] = o.detach().numpy().copy()
            out[pre + 'grad/feature'], out[pre + 'grad/query'] = f.grad.numpy().copy(), q.grad.numpy().copy()
            for k, p in mod.named_parameters():
                out[pre + 'grad/param/' + k] = p.grad.detach().numpy().copy()
    np.savez_compressed(os.path.join(OUT, 'layer_cand_attn.npz'), **out)
    print('layer_cand_attn: %d arrays' % len(out))


def catt_cases():
    """The CATT user encoder (userEncoders.py:194-221) under the CNE and CNN news encoders (`python tools/make_goldens.py catt`).  The tiny CNE
    case must hold users without any history (uniform attention over the padded slots); with the reference's own initialisation CATT's
    gradients are 0.3 % of the total norm, hence gain 2.0 for the CNN case too."""
    with stable_sort_patch():
        cfg = tiny_cfg('CNE', 'CATT')
        run_case('tiny_CNE_CATT_stable', cfg, tiny_spec(cfg, 3), batch_size=8, seed=19, mode='train', gain=2.0)
        lens = np.load(os.path.join(OUT, 'tiny_CNE_CATT_stable.npz'))['in/user_history_mask'].astype(bool).sum(axis=1)
        assert int((lens == 0).sum()) >= 2 and int(lens.max()) >= 4, lens
        print('tiny_CNE_CATT_stable history lengths', lens.tolist())
        cfg = full_cfg('CNE', 'CATT', V=400)
        run_case('full_CNE_CATT_g1p0_stable', cfg, full_spec(cfg, 9), batch_size=2, seed=17, mode='train', gain=1.0, full_arrays=False)
    cfg = tiny_cfg('CNN', 'CATT')
    run_case('tiny_CNN_CATT', cfg, tiny_spec(cfg, 3), batch_size=3, seed=11, mode='train', gain=2.0)
    layer_cand_attn()


class cuda_identity_patch:
    """torch.Tensor.cuda -> identity (OMAP.initialize() calls it on a plain attribute and drops the result)."""

    def __enter__(self):
        self.orig = torch.Tensor.cuda
        torch.Tensor.cuda = lambda self, *a, **k: self

    def __exit__(self, *a):
        torch.Tensor.cuda = self.orig


def omap_cases():
    """The OMAP user encoder (userEncoders.py:335-375) under the CNE and CNN news encoders (`python tools/make_goldens.py omap`), reference
    flag defaults (3 heads, coefficient 0.1).  Weights come from make_state, not from the reference's orthogonal initialisation: there the
    regulariser's norm is fp32 rounding noise and its gradient a noise direction.  The tiny CNE case must hold users without history
    (alpha = 1/H) and padded rows (beta = 1/K).  Every fixture must make the auxiliary term and W's gradient count: asserted below.
    The full-size case runs at gain 0.35, not 1.0: an archive sums 50 history rows, so at gain 1.0 max|user_rep| is 5.06 and the reference's
    own fp32 forward is 2.4e-6 (5-6 ulp) away from float64 -- over the absolute 1e-6 at which tests/test_omap_host.py pins the restatement to
    it.  max|user_rep| is 4.95 x gain (measured at 0.5 ... 1.0); below 2 six ulp are 7e-7, hence a gain under 0.40."""
    omap = dict(OMAP_head_num=3, HiFi_Ark_regularizer_coefficient=0.1)

    def check(tag):
        z = np.load(os.path.join(OUT, tag + '.npz'))
        aux, loss = float(z['auxiliary_loss']), float(z['loss'])
        click = loss - aux
        share = float(z['gradnorm/user_encoder.W']) / float(z['grad_total_norm'])
        print('%s: click loss %.4f, auxiliary term %.4f (%.2fx), |dW| / |g| = %.3f' % (tag, click, aux, aux / click, share))
        assert 0.05 * click <= aux <= 2.0 * click, (tag, aux, click)
        assert share >= 0.01, (tag, share)

    with cuda_identity_patch():
        with stable_sort_patch():
            cfg = tiny_cfg('CNE', 'OMAP', **omap)
            run_case('tiny_CNE_OMAP_stable', cfg, tiny_spec(cfg, 3), batch_size=8, seed=19, mode='train', gain=2.0)
            lens = np.load(os.path.join(OUT, 'tiny_CNE_OMAP_stable.npz'))['in/user_history_mask'].astype(bool).sum(axis=1)
            assert int((lens == 0).sum()) >= 2 and int(lens.max()) >= 4, lens
            print('tiny_CNE_OMAP_stable history lengths', lens.tolist())
            check('tiny_CNE_OMAP_stable')
            cfg = full_cfg('CNE', 'OMAP', V=400, **omap)
            run_case('full_CNE_OMAP_g0p35_stable', cfg, full_spec(cfg, 9), batch_size=2, seed=17, mode='train', gain=0.35, full_arrays=False)
            check('full_CNE_OMAP_g0p35_stable')
        cfg = tiny_cfg('CNN', 'OMAP', **omap)
        run_case('tiny_CNN_OMAP', cfg, tiny_spec(cfg, 3), batch_size=3, seed=11, mode='train', gain=2.0)
        check('tiny_CNN_OMAP')


def npa_cases():
    """NPA (`python tools/make_goldens.py npa`): the PNE news encoder (newsEncoders.py:332-363) and the PUE user encoder
    (userEncoders.py:265-284), together and each with an encoder that ignores the user, on the user-id embedding path of model.py:79-85,
    110-112, 122-125.  make_state weights, as the CATT cases.  The tiny cases have 6 users and a user_ID with a repeated id and id 0 (the
    table has no padding_idx: row 0 takes gradient); user_embedding_dim 6 and personalized_embedding_dim 10 are no multiples of 4.
    Asserted below: the fixtures discriminate -- in the tiny cases the table's, the dense layers' and the personalised attentions' gradients
    are each at least 1 % of the total norm (the full-size case cannot reach that at gain 1.0, see check), and pairing title row r with user r // news_num instead of the reference's r % B (newsEncoders.py:359)
    misses cand_rep by more than 1e-3."""
    from npa_ref import pne_title_rep
    tiny = dict(user_embedding_dim=6, personalized_embedding_dim=10)

    def check(tag, cfg, gain, seed):
        z = np.load(os.path.join(OUT, tag + '.npz'))
        total = float(z['grad_total_norm'])
        watched = [k[len('gradnorm/'):] for k in z.files if k.startswith('gradnorm/') and not k.startswith('gradnorm/user_encoder.news_encoder.')
                   and ('user_embedding.weight' in k or '.dense.' in k or '.personalizedAttention.' in k) and not k.endswith('.bias')]
        assert 'user_embedding.weight' in watched and len(watched) >= 4, watched
        # full dimensions at gain 1.0: the user rows are 0.1 N(0, 1) over 50 columns against conv outputs of O(1), so the query side carries
        # 0.02-0.3 % of the norm whatever the seed (measured at four); there the floor is the 1e-4 from which the model tests compare a
        # gradient's direction, and the 1 % floor is the tiny fixtures', whose every gradient is stored in full
        floor = 0.01 if tag.startswith('tiny_') else 1e-4
        for k in watched:
            share = float(z['gradnorm/' + k]) / total
            print('  %s: |g| / |g_total| = %.4f' % (k, share))
            assert share >= floor, (tag, k, share)
        if cfg.news_encoder == 'PNE':
            B, N = z['in/news_title_text'].shape[:2]
            from nnr_amd.model import Model     # (the reference's parameter names and shapes: tests/test_npa_host.py)
            st = make_state({k: tuple(v.shape) for k, v in Model(cfg, torch.zeros(cfg.vocabulary_size, cfg.word_embedding_dim)).named_parameters()}, seed, gain)
            rows = st['user_embedding.weight'][z['in/user_ID']]
            C = cfg.cnn_kernel_num
            mask = z['mutated_news_title_mask'].reshape(B * N, -1)
            exact = pne_title_rep(z['pne/c_cand'], rows, st, B, N, mask=mask).numpy()
            wrong = pne_title_rep(z['pne/c_cand'], rows, st, B, N, mask=mask, intended=True).numpy()
            e0 = float(np.abs(exact - z['cand_rep'].reshape(B * N, -1)[:, :C]).max())
            e1 = float(np.abs(wrong - z['cand_rep'].reshape(B * N, -1)[:, :C]).max())
            print('  %s: restatement %.2e from cand_rep, with the intended pairing r // news_num %.2e' % (tag, e0, e1))
            assert e0 <= 1e-6 and e1 > 1e-3, (tag, e0, e1)

    def run(tag, cfg, spec, batch_size, seed, gain, ids, **kw):
        run_case(tag, cfg, spec, batch_size=batch_size, seed=seed, mode='train', gain=gain, user_ids=ids, **kw)
        if tag.startswith('tiny_'):
            assert 0 in ids and len(set(ids)) < len(ids), ids
        check(tag, cfg, gain, seed)

    cfg = tiny_cfg('PNE', 'PUE', **tiny)
    cfg.user_num = 6
    run('tiny_PNE_PUE', cfg, tiny_spec(cfg, 3), 5, 19, 2.0, [3, 0, 5, 3, 1])
    cfg = tiny_cfg('PNE', 'ATT', **tiny)
    cfg.user_num = 6
    run('tiny_PNE_ATT', cfg, tiny_spec(cfg, 3), 3, 29, 2.0, [2, 0, 2])
    cfg = tiny_cfg('CNN', 'PUE', **tiny)
    cfg.user_num = 6
    run('tiny_CNN_PUE', cfg, tiny_spec(cfg, 3), 3, 31, 2.0, [4, 4, 0])
    cfg = full_cfg('PNE', 'PUE', V=400, user_num=4, user_embedding_dim=50, personalized_embedding_dim=200)
    run('full_PNE_PUE_g1p0', cfg, full_spec(cfg, 9), 2, 17, 1.0, [3, 0], full_arrays=False)


def bow_cases():
    """The bag-of-words news encoders (`python tools/make_goldens.py bow`): DAE (newsEncoders.py:366-394; Alpha 0.1, config.py:76) and
    Inception (newsEncoders.py:397-433; the three embedding dimensions must be equal: 16) under the ATT and CATT user encoders.
    make_state weights (gain 2.0 tiny, 1.0 full: the reference's own fp32 results there stay inside the model tests' bars), three Adam steps.  The
    synthetic corpus has news with an empty abstract (never an empty title, so DAE's 0 / 0 does not occur).  The DAE fixtures also hold the reconstruction term of each encoder call: `auxiliary_loss` is the LAST call's, the history
    call's.  The tiny fixtures also hold step 0 of a float64 run of the same reference classes (`f64/...`), to which tests/test_bow_host.py pins
    the restatement tensor by tensor.  Asserted below on the tiny cases: the dense layers and the word table each carry at least 1 % of the total gradient norm, and
    for DAE the term is at least 1 % of the loss and the candidate call's value is more than 1e-3 away from the stored one."""
    def check(tag, cfg):
        z = np.load(os.path.join(OUT, tag + '.npz'))
        total = float(z['grad_total_norm'])
        dense = ('f1', 'f2') if cfg.news_encoder == 'DAE' else ('fc1_1', 'fc1_2', 'fc1_3', 'fc2', 'linear_transform')
        for k in ['news_encoder.%s.weight' % d for d in dense] + ['news_encoder.word_embedding.weight']:
            share = float(z['gradnorm/' + k]) / total
            print('  %s: |g| / |g_total| = %.4f' % (k, share))
            assert not tag.startswith('tiny_') or share >= 0.01, (tag, k, share)
        if cfg.news_encoder == 'DAE':
            aux, loss, cand = float(z['auxiliary_loss']), float(z['loss']), float(z['dae/aux_cand'])
            print('  %s: loss %.4f, auxiliary term %.4f (history call) / %.4f (candidate call)' % (tag, loss, aux, cand))
            assert abs(aux - float(z['dae/aux_hist'])) < 1e-7 and aux >= 0.01 * loss and abs(cand - aux) > 1e-3, (tag, aux, loss, cand)

    inc = dict(category_embedding_dim=16, subCategory_embedding_dim=16)
    # seeds: the first of those tried whose candidate-call term is more than 1e-3 from the stored one.  DAE + CATT needs more care: DAE's
    # features are sigmoids, all positive, so a CATT affine1 unit is mostly dead or active for EVERY history slot, and the candidate columns
    # and the bias of an always-active unit (like affine2.bias) have a gradient of exactly zero on paper -- the softmax over the slots does not
    # see a shift common to all of them.  In fp32 those elements are rounding noise of 1e-9 that Adam divides by itself, and three steps walk
    # them in a noise direction in any implementation.  Of the (seed, corpus seed, batch) triples run through the reference in fp32 and in
    # float64 (16 at batch 4, 24 at batch 8), (41, 4) at batch 8 has the fewest such elements among those with the 1e-3 gap: 16 + 1, one
    # unit (the others 32 - 80)
    for tag, news, user, kw, bs, seed, sseed in (('tiny_DAE_ATT', 'DAE', 'ATT', dict(Alpha=0.1), 3, 31, 3), ('tiny_DAE_CATT', 'DAE', 'CATT', dict(Alpha=0.1), 8, 41, 4),
                                                 ('tiny_Inception_ATT', 'Inception', 'ATT', inc, 3, 11, 3), ('tiny_Inception_CATT', 'Inception', 'CATT', inc, 4, 13, 3)):
        cfg = tiny_cfg(news, user, **{k: v for k, v in kw.items() if k == 'Alpha'})
        vars(cfg).update(kw)                    # (tiny_cfg fixes the two category dimensions at 4)
        run_case(tag, cfg, tiny_spec(cfg, sseed), batch_size=bs, seed=seed, mode='train', gain=2.0, f64_step=True)
        check(tag, cfg)
    cfg = full_cfg('DAE', 'ATT', V=400, Alpha=0.1)
    run_case('full_DAE_ATT_g1p0', cfg, full_spec(cfg, 9), batch_size=2, seed=17, mode='train', gain=1.0, full_arrays=False)
    check('full_DAE_ATT_g1p0', cfg)
    cfg = full_cfg('Inception', 'ATT', V=400, category_embedding_dim=300, subCategory_embedding_dim=300)     # (= word_embedding_dim)
    run_case('full_Inception_ATT_g1p0', cfg, full_spec(cfg, 9), batch_size=2, seed=17, mode='train', gain=1.0, full_arrays=False)
    check('full_Inception_ATT_g1p0', cfg)


KCNN_TINY = dict(entity_size=9, entity_embedding_dim=10, context_embedding_dim=6)     # (neither knowledge dimension a multiple of 4)
KCNN_MARGIN = 1e-3


def kcnn_cases():
    """The KCNN news encoder (`python tools/make_goldens.py kcnn`; newsEncoders.py:203-241) under the CATT and ATT user encoders, make_state
    weights (gain 2.0 tiny, 1.0 full), three Adam steps.  The reference's KCNN unpickles both knowledge tables from the working directory:
    build_reference_model writes random ones beside the word table.  The batches get entity ids (tests/kcnn_ref.py:fill_entities): non-zero
    on about a fifth of the positions, 9 distinct ids (repeats across titles), a quarter of the titles without any.  The tiny fixtures also
    hold step 0 of a float64 run of the same classes with the raw convolution outputs of both calls.  Asserted below on the tiny cases: in
    that float64 run every (title, channel) with a positive maximum has its runner-up at least KCNN_MARGIN of the tensor's scale below it
    (an fp32 argmax flip cannot excuse a mismatch; tests/test_kcnn_host.py asserts the same) -- the runner-up among the positions whose window
    has other content: an all-PAD history slot has identical interior windows, equal in any precision and interchangeable --, some maxima sit at the first and at the last
    pooled position and some (title, channel) pairs have none; the convolution, both projections and all three tables each carry at least
    1 % of the total gradient norm.  Seeds: the first of those tried that pass."""
    from kcnn_ref import margins

    def check(tag, cfg):
        z = np.load(os.path.join(OUT, tag + '.npz'))
        total = float(z['grad_total_norm'])
        for k in ('knowledge_cnn.conv.weight', 'M_entity.weight', 'M_context.weight', 'word_embedding.weight', 'entity_embedding.weight', 'context_embedding.weight'):
            share = float(z['gradnorm/news_encoder.' + k]) / total
            print('  %s: |g| / |g_total| = %.4f' % (k, share))
            assert not tag.startswith('tiny_') or share >= 0.01, (tag, k, share)
        ent = np.concatenate([z['in/news_title_entity'].reshape(-1, cfg.max_title_length), z['in/user_title_entity'].reshape(-1, cfg.max_title_length)])
        print('  %s: entity ids on %.3f of the positions, %d of %d titles without any' % (tag, float((ent != 0).mean()), int((ent != 0).sum(1).__eq__(0).sum()), len(ent)))
        assert 0.1 <= float((ent != 0).mean()) <= 0.3 and int(((ent != 0).sum(1) == 0).sum()) >= 2
        if not tag.startswith('tiny_'):
            return True
        ok = True
        for call, pre in (('cand', 'news'), ('hist', 'user')):
            zz = torch.from_numpy(z['f64/kcnn/z_' + call])
            top, gap, arg = margins(zz, cfg.cnn_window_size, z['in/%s_title_text' % pre], z['in/%s_title_entity' % pre])
            scale = float(torch.relu(zz).max())
            worst = float(gap[top > 0].min()) / scale
            T = zz.shape[1] - cfg.cnn_window_size + 1
            arg = arg[top > 0]
            print('  %s %s: smallest margin %.2e of the scale %.3f; maxima at t = 0: %d, at t = %d: %d, none: %d' %
                  (tag, call, worst, scale, int((arg == 0).sum()), T - 1, int((arg == T - 1).sum()), int((top <= 0).sum())))
            ok = ok and worst >= KCNN_MARGIN and (call == 'cand' or (int((arg == 0).sum()) > 0 and int((arg == T - 1).sum()) > 0 and int((top <= 0).sum()) > 0))
        return ok

    for tag, user, bs, seed, sseed in (('tiny_KCNN_CATT', 'CATT', 4, KCNN_SEEDS['tiny_KCNN_CATT'], 3), ('tiny_KCNN_ATT', 'ATT', 3, KCNN_SEEDS['tiny_KCNN_ATT'], 3)):
        cfg = tiny_cfg('KCNN', user, **KCNN_TINY)
        run_case(tag, cfg, tiny_spec(cfg, sseed), batch_size=bs, seed=seed, mode='train', gain=2.0, f64_step=True, entity_seed=seed + 1)
        assert check(tag, cfg), tag
    cfg = full_cfg('KCNN', 'CATT', V=400, entity_size=50, entity_embedding_dim=100, context_embedding_dim=100)
    run_case('full_KCNN_CATT_g1p0', cfg, full_spec(cfg, 9), batch_size=2, seed=17, mode='train', gain=1.0, full_arrays=False, entity_seed=18)
    check('full_KCNN_CATT_g1p0', cfg)


FIM_TINY = dict(click_predictor='FIM', HDC_window_size=3, HDC_filter_num=6, conv3D_filter_num_first=3, conv3D_kernel_size_first=3,
                conv3D_filter_num_second=2, conv3D_kernel_size_second=3)
FIM_FULL = dict(click_predictor='FIM', HDC_window_size=3, HDC_filter_num=150, conv3D_filter_num_first=32, conv3D_kernel_size_first=3,
                conv3D_filter_num_second=16, conv3D_kernel_size_second=3, maxpooling3D_size=3, maxpooling3D_stride=3)
FIM_MARGIN_FACTOR = 20.0
FIM_SEEDS = {'tiny_HDC_FIM': 61, 'tiny_HDC_FIM_p3': 65}       # (p3: 61, 62 and 64 miss the margin; 63 draws a batch whose every cell ties)


def gru_cases():
    """The GRU user encoder (`python tools/make_goldens.py gru`; userEncoders.py:287-332) under the DAE, CNN and CNE news encoders, make_state
    weights (gain 2.0 tiny, 1.0 full: matrices AND biases are drawn at random -- with initialize()'s zero biases an empty user's tanh(dec.bias)
    would be zero like the reference's zero rows), three Adam steps.  Every tiny batch holds a user without history and one with a full history:
    the batch seed is the first from the starting value for which it does.  Asserted below: those two users, max|tanh(dec.bias)| > 1e-2, and that
    the encoder's own parameters carry at least 1 % of the total gradient norm."""
    def pick(cfg, sseed, bs, seed):
        while True:
            lens = SynthCorpus(tiny_spec(cfg, sseed)).batch(bs, np.random.default_rng(seed + 100))['user_history_mask'].sum(axis=1)
            if (lens == 0).any() and (lens == cfg.max_history_num).any():
                return seed
            seed += 1

    def check(tag, tiny):
        z = np.load(os.path.join(OUT, tag + '.npz'))
        lens = z['in/user_history_mask'].astype(bool).sum(axis=1)
        total = float(z['grad_total_norm'])
        share = {k: float(z['gradnorm/user_encoder.' + k]) / total for k in ('gru.weight_ih_l0', 'gru.weight_hh_l0', 'dec.weight')}
        print('  %s: history lengths %s, |g| / |g_total| %s, %d bytes' % (tag, lens.tolist(), {k: round(v, 4) for k, v in share.items()},
                                                                       os.path.getsize(os.path.join(OUT, tag + '.npz'))))
        if tiny:
            assert (lens == 0).any() and (lens == z['in/user_history_mask'].shape[1]).any(), lens
            assert float(np.abs(np.tanh(z['param1/user_encoder.dec.bias'])).max()) > 1e-2
            assert min(share.values()) >= 0.01, share

    for tag, news, kw, bs, seed, sseed in (('tiny_DAE_GRU', 'DAE', dict(Alpha=0.1), 8, 43, 4), ('tiny_CNN_GRU', 'CNN', {}, 8, 11, 3),
                                           ('tiny_CNE_GRU_h48', 'CNE', dict(hidden_dim=48, category_embedding_dim=50, subCategory_embedding_dim=50), 8, 31, 5)):
        cfg = tiny_cfg(news, 'GRU', **{k: v for k, v in kw.items() if k == 'Alpha'})
        vars(cfg).update(kw)
        seed = pick(cfg, sseed, bs, seed)
        # (CNE at hidden_dim 48: the word table's gradient alone is 1.6 MB -- 64-element slices there, as for tiny_CNE_SUE_h48_stable)
        run_case(tag, cfg, tiny_spec(cfg, sseed), batch_size=bs, seed=seed, mode='train', gain=1.5 if news == 'CNE' else 2.0, full_arrays=news != 'CNE')
        check(tag, True)
    cfg = full_cfg('DAE', 'GRU', V=400, Alpha=0.1)
    run_case('full_DAE_GRU_g1p0', cfg, full_spec(cfg, 9), batch_size=2, seed=17, mode='train', gain=1.0, full_arrays=False)
    check('full_DAE_GRU_g1p0', False)


def fim_margin(z):
    """(M, smallest margin, tied cells, cells) of a tiny FIM fixture: M = FIM_MARGIN_FACTOR x the largest deviation of the reference's own
    fp32 convolution outputs from its float64 run; the margin is the smallest gap, over both layers' pool cells, between a cell's maximum
    and a competitor that is not exactly equal to it, relative to the layer's largest absolute output (tests/fim_ref.py:pool_margins)."""
    from fim_ref import pool_margins
    meta = dict(zip(z['meta_keys'].tolist(), z['meta_vals'].tolist()))
    P, St = int(meta['maxpooling3D_size']), int(meta['maxpooling3D_stride'])
    res = [pool_margins(z['f64/fim/' + k], P, St) for k in ('za', 'zb')]
    return FIM_MARGIN_FACTOR * float(z['fim/conv_dev']), min(r[0] for r in res), [r[1] for r in res], [r[2] for r in res]


def fim_cases(search=False):
    """The FIM baseline (`python tools/make_goldens.py fim`): HDC news encoder, FIM user encoder and click head, make_state weights
    (gain 2.0 tiny, 1.0 full).  tiny_HDC_FIM: history 11, title 10 (S = 12), pool 2 / 2: 11 x 12 x 12 -> 9 x 10 x 10 -> 4 x 5 x 5 (the first
    pool drops a remainder along the history axis) -> 2 x 3 x 3 -> 1 x 1 x 1; three Adam steps with the float64 step.  tiny_HDC_FIM_p3: the
    default pool 3 / 3 at history 17, title 17 (S = 19, a remainder of 2): the smallest extents that leave one cell after both layers.
    Asserted on the tiny cases: in the float64 run every pool maximum beats every competitor that is not exactly equal to it by M (see
    fim_margin); exact ties are counted and printed (a padded history slot repeats its neighbour's window).  Seeds: the first from 61 that pass
    (`python tools/make_goldens.py fim search` prints the margins of the seeds it tries)."""
    cases = (('tiny_HDC_FIM', dict(max_history_num=11, max_title_length=10, maxpooling3D_size=2, maxpooling3D_stride=2), 2, 3),
             ('tiny_HDC_FIM_p3', dict(max_history_num=17, max_title_length=17, maxpooling3D_size=3, maxpooling3D_stride=3), 1, 3))
    for tag, over, bs, steps in cases:
        seeds = range(61, 71) if search else (FIM_SEEDS[tag],)
        for seed in seeds:
            cfg = tiny_cfg('HDC', 'FIM', **FIM_TINY)
            vars(cfg).update(over)
            out_tag = tag + '_search' if search else tag          # (a search leaves the committed fixtures alone)
            run_case(out_tag, cfg, tiny_spec(cfg, 3), batch_size=bs, seed=seed, mode='train', gain=2.0, adam_steps=steps, f64_step=True)
            z = np.load(os.path.join(OUT, out_tag + '.npz'))
            if search:
                z = {k: z[k] for k in z.files}
                os.remove(os.path.join(OUT, out_tag + '.npz'))
            M, worst, tied, cells = fim_margin(z)
            total = float(z['grad_total_norm'])
            shares = {k: float(z['gradnorm/' + k]) / total for k in ('user_encoder.conv_3D_a.weight', 'user_encoder.conv_3D_b.weight',
                      'news_encoder.dilated_conv1.weight', 'news_encoder.layer_norm3.weight', 'news_encoder.word_embedding.weight', 'fc.weight')}
            print('  %s seed %d: fp32 deviation %.2e -> M = %.2e; smallest margin %.2e; tied cells %s of %s; shares %s' %
                  (tag, seed, float(z['fim/conv_dev']), M, worst, tied, cells, {k.split('.', 1)[1]: round(v, 4) for k, v in shares.items()}))
            ok = worst >= M and min(shares.values()) >= 0.01
            if not search:
                assert ok, (tag, seed, M, worst, shares)
            elif ok:
                print('  -> %s: seed %d passes' % (tag, seed))
                break
    if search:
        return
    cfg = full_cfg('HDC', 'FIM', V=400, **FIM_FULL)
    run_case('full_HDC_FIM_g1p0', cfg, full_spec(cfg, 9), batch_size=2, seed=17, mode='train', gain=1.0, full_arrays=False, adam_steps=1)


NAML_MARGIN = 1e-3
NAML_SEEDS = {'tiny_NAML_Title_ATT': 81, 'tiny_NAML_Content_ATT': 84, 'tiny_NAML_Content_CATT': 84}      # (searched from 71: 10, 13 and 13 seeds miss the margin)


def naml_margin(z):
    """Smallest |relu pre-activation| of a tiny NAML fixture's float64 run over its tensor's scale (max |.|), over the convolution outputs and
    both category affines of both encoder calls."""
    return min(float(np.abs(z[k]).min() / np.abs(z[k]).max()) for k in z.files if k.startswith('f64/naml/'))


def naml_cases(search=False):
    """The single-view NAML news encoders (`python tools/make_goldens.py naml`; variantEncoders.py:102-187) under the ATT and CATT user
    encoders, make_state weights (gain 2.0 tiny, 1.0 full: matrices AND biases drawn at random -- initialize()'s zero biases would hide the
    bias paths), three Adam steps.  No dataset override of dropout applies (the cases set it).  The tiny fixtures also hold step 0 of a
    float64 run of the same classes with the relu pre-activations of both calls (`f64/naml/...`: convolution outputs [n L, C], category and
    subCategory affines [n, C]).  Asserted below on the tiny cases: in that float64 run no pre-activation lies within NAML_MARGIN of its
    tensor's scale of zero (an fp32 sign flip cannot excuse a mismatch; tests/test_naml_host.py asserts the same), and the convolution, the
    four view-attention matrices and the word table each carry at least 1 % of the total gradient norm.  Seeds: the first from the starting
    value that pass (`python tools/make_goldens.py naml search` prints the margins of the seeds it tries).
    drop_tiny_NAML_Content_ATT: the reference in train mode at dropout 0.25 with its masks recorded (record_dropout): four calls, the word
    rows and the convolution output of the candidate call, then of the history call."""
    def check(tag):
        z = np.load(os.path.join(OUT, tag + '.npz'))
        total = float(z['grad_total_norm'])
        names = [k[len('gradnorm/'):] for k in z.files if k.startswith('gradnorm/news_encoder.') and k.endswith('.weight') and 'Category_embedding' not in k
                 and 'category_embedding' not in k]
        shares = {k.split('.', 1)[1]: float(z['gradnorm/' + k]) / total for k in names}
        margin = naml_margin(z) if tag.startswith('tiny_') else float('nan')
        print('  %s: smallest relu margin %.2e of the scale; shares %s; %d bytes' % (tag, margin, {k: round(v, 4) for k, v in shares.items()},
                                                                                  os.path.getsize(os.path.join(OUT, tag + '.npz'))))
        return not tag.startswith('tiny_') or (margin >= NAML_MARGIN and min(shares.values()) >= 0.01)

    for tag, news, user, bs, first, sseed in (('tiny_NAML_Title_ATT', 'NAML_Title', 'ATT', 3, 71, 3), ('tiny_NAML_Content_ATT', 'NAML_Content', 'ATT', 3, 71, 3),
                                              ('tiny_NAML_Content_CATT', 'NAML_Content', 'CATT', 4, 71, 3)):
        seeds = range(first, first + 200) if search else (NAML_SEEDS[tag],)
        for seed in seeds:
            cfg = tiny_cfg(news, user)
            out_tag = tag + '_search' if search else tag          # (a search leaves the committed fixtures alone)
            run_case(out_tag, cfg, tiny_spec(cfg, sseed), batch_size=bs, seed=seed, mode='train', gain=2.0, f64_step=True)
            ok = check(out_tag)
            if search:
                os.remove(os.path.join(OUT, out_tag + '.npz'))
                if ok:
                    print('  -> %s: seed %d passes' % (tag, seed))
                    break
            else:
                assert ok, (tag, seed)
    if search:
        return
    cfg = tiny_cfg('NAML_Content', 'ATT')
    cfg.dropout_rate = 0.25
    run_case('drop_tiny_NAML_Content_ATT', cfg, tiny_spec(cfg, 8), batch_size=3, seed=47, mode='train', gain=2.0, adam_steps=1, dropout_seed=5)
    z = np.load(os.path.join(OUT, 'drop_tiny_NAML_Content_ATT.npz'))
    assert z['drop_p'].tolist() == [0.25] * 4 and [int(z['drop_shape/%d' % i][-1]) for i in range(4)] == [cfg.word_embedding_dim, cfg.cnn_kernel_num] * 2
    cfg = full_cfg('NAML_Title', 'ATT', V=400)
    run_case('full_NAML_Title_ATT_g1p0', cfg, full_spec(cfg, 9), batch_size=2, seed=17, mode='train', gain=1.0, full_arrays=False)
    check('full_NAML_Title_ATT_g1p0')


def sue_ablation_conditions(z):
    """The four conditions a tiny sue_ablation batch must meet (tests/test_sue_ablation_host.py asserts the same): a user without history and
    one with a full history; a cluster with at least two members; a cluster that is empty but unmasked (the mask as SUE_wo_GCN reads it: last
    column set); clusterFeatureAffine.bias / the proxy nodes visibly non-zero."""
    hm = z['in/user_history_mask'].astype(bool)
    cidx = z['in/user_history_category_indices']
    cmask = z['in/user_history_category_mask'].astype(bool).copy()
    cmask[:, -1] = True
    lens = hm.sum(axis=1)
    counts = np.stack([(cidx == c).sum(axis=1) for c in range(cmask.shape[1])], axis=1)          # [B, category_num + 1]
    pre = 'param1/user_encoder.'
    big = [float(np.abs(z[pre + k]).max()) for k in ('clusterFeatureAffine.bias', 'proxy_node_embedding') if pre + k in z.files]
    return dict(empty_user=bool((lens == 0).any()), full_user=bool((lens == hm.shape[1]).any()), multi_member=bool((counts >= 2).any()),
                empty_unmasked=bool(((counts == 0) & cmask).any()), visible=bool(big) and min(big) > 1e-2), lens


def sue_ablation_cases():
    """The user-encoder ablations of the paper's own model (`python tools/make_goldens.py sue_ablation`; variantEncoders.py:342-419):
    SUE_wo_GCN and SUE_wo_HCA under the CNN and CNE news encoders, make_state weights (gain 2.0 tiny, 1.0 full: matrices AND biases drawn at
    random, so clusterFeatureAffine.bias and the proxy nodes -- zero after initialize() -- take part), three Adam steps, the tiny cases with
    step 0 of a float64 run of the same classes (`f64/...`).  tiny_CNN_SUE_wo_HCA_ln: --gcn_layer_norm, one Adam step (see extra_cases).
    Every tiny batch meets sue_ablation_conditions: the batch seed is the first from the starting value for which it does (tiny_spec(cfg, 3)
    at batch 8 from seed 19 gives history lengths [2,0,4,0,4,5,0,1]: no full user)."""
    def pick(cfg, sseed, bs, seed):
        while True:
            b = SynthCorpus(tiny_spec(cfg, sseed)).batch(bs, np.random.default_rng(seed + 100))
            ok, _ = sue_ablation_conditions(_NoFiles({'in/' + k: b[k] for k in ('user_history_mask', 'user_history_category_indices',
                                                                                 'user_history_category_mask')}))
            if all(v for k, v in ok.items() if k != 'visible'):
                return seed
            seed += 1

    def check(tag, tiny):
        z = np.load(os.path.join(OUT, tag + '.npz'))
        ok, lens = sue_ablation_conditions(z)
        total = float(z['grad_total_norm'])
        share = {k[len('gradnorm/user_encoder.'):]: round(float(z[k]) / total, 4) for k in z.files
                 if k.startswith('gradnorm/user_encoder.') and not k.startswith('gradnorm/user_encoder.news_encoder.')}
        print('  %s: history lengths %s, %s, |g| / |g_total| %s, %d bytes' % (tag, lens.tolist(), ok, share, os.path.getsize(os.path.join(OUT, tag + '.npz'))))
        assert os.path.getsize(os.path.join(OUT, tag + '.npz')) < 350000, tag
        if tiny:
            assert all(ok.values()), (tag, ok)
        kb = 'grad/user_encoder.intraCluster_K.bias'
        if kb in z.files:
            qmax = float(np.abs(z['grad/user_encoder.intraCluster_Q.bias']).max())
            print('  %s: max|d intraCluster_K.bias| %.2e, max|d intraCluster_Q.bias| %.2e' % (tag, float(np.abs(z[kb]).max()), qmax))
            assert float(np.abs(z[kb]).max()) < 1e-5 * qmax, tag

    for user in ('SUE_wo_GCN', 'SUE_wo_HCA'):
        cfg = tiny_cfg('CNN', user)
        run_case('tiny_CNN_%s' % user, cfg, tiny_spec(cfg, 3), batch_size=8, seed=pick(cfg, 3, 8, 19), mode='train', gain=2.0, f64_step=True)
        check('tiny_CNN_%s' % user, True)
        with stable_sort_patch():
            cfg = tiny_cfg('CNE', user)
            run_case('tiny_CNE_%s_stable' % user, cfg, tiny_spec(cfg, 3), batch_size=8, seed=pick(cfg, 3, 8, 19), mode='train', gain=2.0, f64_step=True)
        check('tiny_CNE_%s_stable' % user, True)
        cfg = full_cfg('CNN', user, V=400)
        run_case('full_CNN_%s_g1p0' % user, cfg, full_spec(cfg, 9), batch_size=2, seed=17, mode='train', gain=1.0, full_arrays=False)
        check('full_CNN_%s_g1p0' % user, False)
    cfg = tiny_cfg('CNN', 'SUE_wo_HCA', gcn_layer_norm=True)
    run_case('tiny_CNN_SUE_wo_HCA_ln', cfg, tiny_spec(cfg, 3), batch_size=8, seed=pick(cfg, 3, 8, 19), mode='train', gain=2.0, adam_steps=1, f64_step=True)
    check('tiny_CNN_SUE_wo_HCA_ln', True)


CNE_ABLATION_PAIR_MOVE = 100 * 2e-5      # a wrong gate partner must move hist_rep by 100 x the GPU tests' output bar
CNE_ABLATION_TINY = (('tiny_CNE_Title_ATT', 'CNE_Title', 'ATT'), ('tiny_CNE_Content_ATT', 'CNE_Content', 'ATT'), ('tiny_CNE_wo_CS_ATT', 'CNE_wo_CS', 'ATT'),
                     ('tiny_CNE_wo_CS_SUE_stable', 'CNE_wo_CS', 'SUE'), ('tiny_CNE_wo_CA_ATT_stable', 'CNE_wo_CA', 'ATT'),
                     ('tiny_CNE_wo_CA_SUE_stable', 'CNE_wo_CA', 'SUE'))


def cne_ablation_empty_title(batch):
    """The synthetic corpus has no news with an all-zero title mask (its PAD news sets position 0, MIND_corpus.py:352-353): the second
    candidate of the first sample and the first history slot of the first user that has one lose theirs, so that the encoders' own
    `title_mask[:, 0] = 1` acts on both calls."""
    batch['news_title_mask'][0, 1, :] = False
    b = int(np.argmax(batch['user_history_mask'][:, 0]))
    assert batch['user_history_mask'][b, 0]
    batch['user_title_mask'][b, 0, :] = False


def cne_ablation_conditions(z):
    """What a tiny cne_ablation batch must hold (tests/test_cne_ablation_host.py asserts the same), per condition over both encoder calls:
    a title with an all-zero mask, a title of full length, a content of length 1, an empty content, two equal lengths above 1 in each stream
    of the history call, and a padded history slot (news 0: one token, id 0)."""
    tm = np.concatenate([z['in/%s_title_mask' % c].reshape(-1, z['in/news_title_mask'].shape[-1]) for c in ('news', 'user')]).astype(bool)
    cm = np.concatenate([z['in/%s_content_mask' % c].reshape(-1, z['in/news_content_mask'].shape[-1]) for c in ('news', 'user')]).astype(bool)

    def tie(mask):
        lens = mask.reshape(-1, mask.shape[-1]).astype(bool).sum(axis=1)
        vals, counts = np.unique(lens[lens > 1], return_counts=True)
        return bool((counts >= 2).any())
    return dict(empty_title=bool((tm.sum(1) == 0).any()), full_title=bool(tm.all(axis=1).any()), content_of_one=bool((cm.sum(1) == 1).any()),
                empty_content=bool((cm.sum(1) == 0).any()), title_tie=tie(z['in/user_title_mask']), content_tie=tie(z['in/user_content_mask']),
                pad_slot=bool((~z['in/user_history_mask'].astype(bool)).any() and (z['in/user_title_text'][~z['in/user_history_mask'].astype(bool)] == 0).all()))


def cne_ablation_cases():
    """The news-encoder ablations of the paper's own model (`python tools/make_goldens.py cne_ablation`; variantEncoders.py:14-99,190-339)
    under the ATT and SUE user encoders, make_state weights (gain 2.0 tiny, 1.0 full), three Adam steps, the tiny cases at batch 8 with step 0
    of a float64 run of the same classes (`f64/...`, with its gradients with respect to the two encoder outputs) and the mutated copies of
    all four text masks.  The `_stable` cases -- every case in which the gate's rank pairing or SUE's inputs depend on the order of equal
    lengths -- run with torch.sort forced stable, as the CNE fixtures do.  Every tiny batch meets cne_ablation_conditions (one title mask of
    each call is cleared by cne_ablation_empty_title), and for CNE_wo_CA pairing the gate by index instead of by sorted rank moves hist_rep by
    at least CNE_ABLATION_PAIR_MOVE (tests/cne_ablation_ref.py, pair='index'): the corpus seed is the first from 3 for which both hold."""
    import cne_ablation_ref as R
    from nnr_amd.model import Model

    def pick(cfg, news, bs, seed, sseed):
        while True:
            b = SynthCorpus(tiny_spec(cfg, sseed)).batch(bs, np.random.default_rng(seed + 100))
            cne_ablation_empty_title(b)
            ok = cne_ablation_conditions({'in/' + k: v for k, v in b.items()})
            move = float('inf')
            if all(ok.values()) and news == 'CNE_wo_CA':
                st = make_state({k: tuple(v.shape) for k, v in Model(cfg, torch.zeros(cfg.vocabulary_size, cfg.word_embedding_dim)).named_parameters()}, seed, 2.0)
                a, c = (R.encode_batch(news, st, cfg, b, pair=pr)['hist_rep'] for pr in ('rank', 'index'))
                move = float((a - c).abs().max())
            print('  corpus seed %d: %s, pair move %.3e' % (sseed, ok, move))
            if all(ok.values()) and move >= CNE_ABLATION_PAIR_MOVE:
                return sseed
            sseed += 1

    def check(tag, tiny):
        z = np.load(os.path.join(OUT, tag + '.npz'))
        total = float(z['grad_total_norm'])
        share = {k[len('gradnorm/news_encoder.'):]: round(float(z[k]) / total, 4) for k in z.files if k.startswith('gradnorm/news_encoder.') and k.endswith('weight')}
        print('  %s: |g| / |g_total| %s, %d bytes' % (tag, share, os.path.getsize(os.path.join(OUT, tag + '.npz'))))
        assert os.path.getsize(os.path.join(OUT, tag + '.npz')) < 350000, tag
        if tiny:
            ok = cne_ablation_conditions(z)
            assert all(ok.values()), (tag, ok)

    for tag, news, user in CNE_ABLATION_TINY:
        cfg = tiny_cfg(news, user)
        sseed = pick(cfg, news, 8, 19, 3)
        kw = dict(batch_size=8, seed=19, mode='train', gain=2.0, f64_step=True, batch_hook=cne_ablation_empty_title, all_masks=True, rep_grads=True)
        if tag.endswith('_stable'):
            with stable_sort_patch():
                run_case(tag, cfg, tiny_spec(cfg, sseed), **kw)
        else:
            run_case(tag, cfg, tiny_spec(cfg, sseed), **kw)
        check(tag, True)
    for tag, news in (('full_CNE_Title_ATT_g1p0', 'CNE_Title'), ('full_CNE_wo_CS_ATT_g1p0', 'CNE_wo_CS'), ('full_CNE_wo_CA_ATT_g1p0_stable', 'CNE_wo_CA')):
        cfg = full_cfg(news, 'ATT', V=400)
        kw = dict(batch_size=2, seed=17, mode='train', gain=1.0, full_arrays=False, all_masks=True)
        if tag.endswith('_stable'):
            with stable_sort_patch():
                run_case(tag, cfg, full_spec(cfg, 9), **kw)
        else:
            run_case(tag, cfg, full_spec(cfg, 9), **kw)
        check(tag, False)


class _NoFiles(dict):
    """A plain dict of batch arrays as sue_ablation_conditions' argument: no stored parameters."""
    files = ()


KCNN_SEEDS = {'tiny_KCNN_CATT': 55, 'tiny_KCNN_ATT': 54}      # (53, 54 and 53 miss the margin: 2.3e-4, 4.3e-4 and 1.8e-4 of the scale)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == 'fim':
        torch.set_num_threads(8)
        return fim_cases(search=len(sys.argv) > 2 and sys.argv[2] == 'search')
    if len(sys.argv) > 1 and sys.argv[1] == 'naml':
        torch.set_num_threads(8)
        return naml_cases(search=len(sys.argv) > 2 and sys.argv[2] == 'search')
    if len(sys.argv) > 1 and sys.argv[1] == 'gru':
        torch.set_num_threads(8)
        return gru_cases()
    if len(sys.argv) > 1 and sys.argv[1] == 'sue_ablation':
        torch.set_num_threads(8)
        return sue_ablation_cases()
    if len(sys.argv) > 1 and sys.argv[1] == 'cne_ablation':
        torch.set_num_threads(8)
        return cne_ablation_cases()
    if len(sys.argv) > 1 and sys.argv[1] == 'kcnn':
        torch.set_num_threads(8)
        return kcnn_cases()
    if len(sys.argv) > 1 and sys.argv[1] == 'bow':
        torch.set_num_threads(8)
        return bow_cases()
    if len(sys.argv) > 1 and sys.argv[1] == 'omap':
        torch.set_num_threads(8)
        return omap_cases()
    if len(sys.argv) > 1 and sys.argv[1] == 'npa':
        torch.set_num_threads(8)
        return npa_cases()
    if len(sys.argv) > 1 and sys.argv[1] == 'catt':
        torch.set_num_threads(8)
        return catt_cases()
    if len(sys.argv) > 1 and sys.argv[1] == 'extra':
        torch.set_num_threads(8)
        return extra_cases()
    if len(sys.argv) > 1 and sys.argv[1] == 'dropout':
        torch.set_num_threads(8)
        return dropout_cases()
    torch.set_num_threads(8)
    # tiny dims, reference's own initialisation, every array stored
    for news, user, mode in (('CNE', 'SUE', 'train'), ('MHSA', 'MHSA', 'eval'), ('CNN', 'ATT', 'train')):
        cfg = tiny_cfg(news, user)
        run_case('tiny_%s_%s' % (news, user), cfg, tiny_spec(cfg, 3), batch_size=3, seed=11, mode=mode)
    # tiny dims, larger weights (logits O(1-10)), still every array stored
    cfg = tiny_cfg('CNE', 'SUE')
    run_case('tiny_CNE_SUE_scaled', cfg, tiny_spec(cfg, 5), batch_size=4, seed=13, mode='train', gain=2.5)
    with stable_sort_patch():
        cfg = tiny_cfg('CNE', 'SUE')
        run_case('tiny_CNE_SUE_stable', cfg, tiny_spec(cfg, 3), batch_size=8, seed=19, mode='train', gain=2.0)
        cfg = full_cfg('CNE', 'SUE', V=400)
        run_case('full_CNE_SUE_g1p0_stable', cfg, full_spec(cfg, 9), batch_size=2, seed=17, mode='train', gain=1.0,
                 full_arrays=False)
    # full model dims at B=2: regenerable weights, outputs + gradient norms + 64-element slices
    for news, user, mode, gain in (('CNE', 'SUE', 'train', 1.0), ('CNE', 'SUE', 'train', 1.6),
                                   ('MHSA', 'MHSA', 'eval', 1.0), ('CNN', 'ATT', 'train', 1.0)):
        cfg = full_cfg(news, user, V=400)
        tag = 'full_%s_%s_g%s' % (news, user, str(gain).replace('.', 'p'))
        run_case(tag, cfg, full_spec(cfg, 9), batch_size=2, seed=17, mode=mode, gain=gain, full_arrays=False)


if __name__ == '__main__':
    main()
