"""The user-encoder ablations SUE_wo_GCN / SUE_wo_HCA on the GPU: the segmented candidate pool in GEMV form (csrc/sue_cluster.hip)
against the float64 restatement (tests/sue_ablation_ref.py, pinned to the reference by tests/test_sue_ablation_host.py), its edge rules and
reproducibility; both encoders on random inputs with dropout off and on (the kernels' own keep-masks handed to the restatement); and the
model / evaluation paths against golden vectors captured from the reference's own code.  Bars as in tests/test_hip_catt_gpu.py."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sue_ablation_ref as R
from golden_io import GoldenCase, build_model, eval_fixture

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4
TIGHT = 2e-5            # outputs, absolute (inputs scaled so that outputs are O(1))
GRAD = 5e-5             # each gradient, of its own largest magnitude
CASES = ['tiny_CNN_SUE_wo_GCN', 'tiny_CNN_SUE_wo_HCA', 'tiny_CNE_SUE_wo_GCN_stable', 'tiny_CNE_SUE_wo_HCA_stable', 'full_CNN_SUE_wo_GCN_g1p0',
         'full_CNN_SUE_wo_HCA_g1p0', 'tiny_CNN_SUE_wo_HCA_ln']
# (B, N, Hn, C, D): odd D below one wave | B no multiple of 8, a partial last column pass | N = 1, the evaluation shape | all three limits |
# Hn <= C, for the one-item-per-cluster pattern
KERNEL_CASES = [((3, 2, 6, 4, 7), 'random', 1.0), ((3, 2, 6, 4, 7), 'one_cluster', 1.0), ((3, 2, 6, 4, 7), 'random', 80.0),
                ((9, 5, 50, 19, 300), 'random', 1.0), ((9, 5, 50, 19, 300), 'empty_ends', 1.0), ((9, 5, 50, 19, 300), 'last_user', 1.0),
                ((2, 1, 50, 19, 900), 'random', 1.0), ((2, 1, 50, 19, 900), 'one_cluster', 1.0),
                ((2, 8, 64, 32, 33), 'random', 1.0), ((2, 8, 64, 32, 33), 'empty_ends', 1.0), ((2, 8, 64, 32, 33), 'last_user', 1.0),
                ((2, 3, 5, 8, 12), 'one_per_cluster', 1.0)]


def _clusters(B, Hn, C, pattern, g):
    if pattern == 'one_cluster':
        return torch.full((B, Hn), C // 2, dtype=torch.int64)
    if pattern == 'one_per_cluster':
        return torch.stack([torch.randperm(C, generator=g)[:Hn] for _ in range(B)])
    if pattern == 'empty_ends':                                   # the first and the last cluster stay empty
        return torch.randint(1, C - 1, (B, Hn), generator=g)
    cidx = torch.randint(0, C, (B, Hn), generator=g)
    if pattern == 'last_user':                                    # a user whose items all sit in the last cluster (a user without history)
        cidx[0] = C - 1
    return cidx


@functools.lru_cache(maxsize=None)
def _kernel_problem(shape, pattern, mag):
    """fp32 inputs and the float64 expectation, computed once.  scale = 1 / sqrt(D) with N(0, 1) rows: scores of O(1), outputs of O(1).
    mag > 1: every row of x and u gets the same offset along the all-ones direction, sized so that it adds `mag` to every score: the scores
    are about mag, their spread inside a cluster stays a few units (pure scaling makes every softmax one-hot and every score gradient
    zero), and the features stay below 10."""
    B, N, Hn, C, D = shape
    g = torch.Generator().manual_seed(sum(shape) + len(pattern) + int(mag))
    x, u = torch.randn(B, Hn, D, generator=g), torch.randn(B, N, D, generator=g)
    scale = 1.0 / D ** 0.5
    if mag > 1.0:
        off = (mag / (scale * D)) ** 0.5                          # scale * D * off^2 = mag
        x, u = x + off, u + off
    cidx = _clusters(B, Hn, C, pattern, g)
    dfeat = torch.randn(B, N, C, D, generator=g)
    xd, ud = R.f64(x).requires_grad_(), R.f64(u).requires_grad_()
    alpha, feat = R.seg_pool(xd, ud, cidx, C, scale)
    (feat * R.f64(dfeat)).sum().backward()
    exp = dict(alpha=alpha.detach(), feat=feat.detach(), dx=xd.grad, du=ud.grad)
    return x, u, cidx, dfeat, scale, exp


def _run_kernel(x, u, cidx, dfeat, scale, C):
    from nnr_amd import ops
    B, Hn, D = x.shape
    N = u.shape[1]
    dev = dict(device='cuda', dtype=torch.float32)
    xd, ud, cd, dfd = x.cuda().contiguous(), u.cuda().contiguous().view(B * N, D), cidx.cuda().contiguous(), dfeat.cuda().contiguous().view(B * N * C, D)
    alpha = torch.full((B, N, Hn), float('nan'), **dev)
    feat = torch.full((B * N * C, D), float('nan'), **dev)
    ops.sue_seg_pool_fwd(xd, ud, cd, B, N, Hn, C, D, scale, alpha, feat)
    dx = torch.full((B, Hn, D), float('nan'), **dev)              # dx is written, not accumulated: every element, whatever was there
    du = torch.full((B * N, D), float('nan'), **dev)
    ops.sue_seg_pool_bwd(xd, ud, cd, alpha, dfd, B, N, Hn, C, D, scale, dx, du)
    torch.cuda.synchronize()
    return dict(alpha=alpha, feat=feat.view(B, N, C, D), dx=dx, du=du.view(B, N, D))


def _check(got, exp, tag, grads):
    report, worst = [], {}
    for k, e in exp.items():
        if not torch.is_tensor(e):
            continue
        a = got[k].detach().cpu().double()
        assert bool(torch.isfinite(a).all()), (tag, k)
        err, emax = float((a - e).abs().max()), float(e.abs().max())
        bar = GRAD * emax if k in grads else TIGHT
        report.append('%s err %.3e (max|exp| %.3e, bar %.3e)' % (k, err, emax, bar))
        worst[k] = (err, bar)
    print(tag + ': ' + '; '.join(report))
    for k, (err, bar) in worst.items():
        assert err <= bar, (tag, k, err, bar)


@pytest.mark.parametrize('shape,pattern,mag', KERNEL_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_kernel_matches_the_float64_restatement(shape, pattern, mag):
    x, u, cidx, dfeat, scale, exp = _kernel_problem(shape, pattern, mag)
    C = shape[3]
    if mag != 1.0:
        s = scale * torch.einsum('bhd,bnd->bnh', x.double(), u.double())
        assert 0.5 * mag <= float(s.abs().max()) <= 4 * mag
    got = _run_kernel(x, u, cidx, dfeat, scale, C)
    _check(got, exp, '%s %s %g' % (shape, pattern, mag), grads=('dx', 'du'))
    # an empty cluster's rows are exactly zero
    present = torch.nn.functional.one_hot(cidx, C).sum(dim=1) > 0                    # [B, C]
    empty = (~present).unsqueeze(1).expand(-1, shape[1], -1)
    if pattern in ('one_cluster', 'empty_ends', 'last_user'):
        assert bool(empty.any())
    assert float(got['feat'].cpu()[empty].abs().sum()) == 0.0


def test_kernels_are_bit_reproducible():
    x, u, cidx, dfeat, scale, _ = _kernel_problem((9, 5, 50, 19, 300), 'random', 1.0)
    a, b = _run_kernel(x, u, cidx, dfeat, scale, 19), _run_kernel(x, u, cidx, dfeat, scale, 19)
    for k in ('alpha', 'feat', 'dx', 'du'):
        assert torch.equal(a[k], b[k]), k


def test_out_of_range_sizes_are_refused_before_any_launch():
    from nnr_amd import ops, _lib
    dev = dict(device='cuda', dtype=torch.float32)
    for B, N, Hn, C, D in ((2, 9, 6, 4, 8), (2, 2, 65, 4, 8), (2, 2, 6, 33, 8), (2, 2, 6, 4, 0), (2, 0, 6, 4, 8)):
        x, u = torch.zeros((B, Hn, max(D, 1)), **dev), torch.zeros((max(B * N, 1), max(D, 1)), **dev)
        cidx = torch.zeros((B, Hn), device='cuda', dtype=torch.int64)
        alpha, feat = torch.full((B, max(N, 1), Hn), 7.0, **dev), torch.full((max(B * N, 1) * C, max(D, 1)), 7.0, **dev)
        dx, du = torch.full_like(x, 7.0), torch.full_like(u, 7.0)
        with pytest.raises(_lib.NnrHipError, match='unsupported size'):
            ops.sue_seg_pool_fwd(x, u, cidx, B, N, Hn, C, D, 1.0, alpha, feat)
        with pytest.raises(_lib.NnrHipError, match='unsupported size'):
            ops.sue_seg_pool_bwd(x, u, cidx, alpha, feat, B, N, Hn, C, D, 1.0, dx, du)
        rc = _lib.lib().nnr_sue_seg_pool_bwd(x.data_ptr(), u.data_ptr(), cidx.data_ptr(), alpha.data_ptr(), feat.data_ptr(), B, N, Hn, C, D, 1.0,
                                             dx.data_ptr(), du.data_ptr(), alpha.data_ptr(), None)
        assert rc == _lib.NNR_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        for t in (alpha, feat, dx, du):                           # nothing ran
            assert bool((t == 7.0).all())


# ------------------------------------------------------------------------------------------------ encoder level
ENC_SHAPES = [(5, 3, 6, 3, 20), (4, 5, 50, 18, 500)]             # (B, N, Hn, K = category_num, D)
RELU_MARGIN = 3e-6      # no relu pre-activation of the float64 run closer to zero than this, relative to its tensor's rms (offending seeds are
                        # passed over), so that an fp32 sign flip cannot excuse a mismatch: ten times the fp32 error of a sum of 500 products
                        # (about 3e-7 of the sum's rms).  The larger SUE_wo_HCA shape has 4 x 68 x 500 x 3 of them: one seed in three keeps it


class _Rows(torch.nn.Module):
    """Stands where the news encoder stands: the encoders under test read its news_embedding_dim only."""

    def __init__(self, D):
        super().__init__()
        self.news_embedding_dim = D


def _enc_cfg(Hn, K, N, p, seed, layers=3):
    return SimpleNamespace(attention_dim=8, category_num=K, max_history_num=Hn, dropout_rate=p, negative_sample_num=N - 1, gcn_layer_num=layers,
                           no_gcn_residual=False, gcn_layer_norm=False, seed=seed)


def _encoder(name, shape, p, seed, layers=3):
    from nnr_amd import user_encoders
    B, N, Hn, K, D = shape
    cfg = _enc_cfg(Hn, K, N, p, seed, layers)
    torch.manual_seed(seed)
    enc = getattr(user_encoders, name)(_Rows(D), cfg)
    enc.initialize()
    with torch.no_grad():                                         # biases and proxy nodes visibly non-zero
        for k, q in enc.named_parameters():
            if q.dim() == 1 or k == 'proxy_node_embedding':
                q.copy_(0.1 * torch.randn(q.shape))
    return enc.cuda().train(), cfg


def _enc_inputs(shape, seed):
    B, N, Hn, K, D = shape
    g = torch.Generator().manual_seed(seed)
    hist, cand, dout = 0.5 * torch.randn(B, Hn, D, generator=g), 0.5 * torch.randn(B, N, D, generator=g), torch.randn(B, N, D, generator=g)
    lens = torch.randint(0, Hn + 1, (B,), generator=g)
    lens[0], lens[1] = 0, Hn
    hmask = torch.arange(Hn).unsqueeze(0) < lens.unsqueeze(1)
    cidx = torch.where(hmask, torch.randint(0, K, (B, Hn), generator=g), torch.full((B, Hn), K))
    cmask = torch.zeros(B, K + 1, dtype=torch.bool)
    cmask.scatter_(1, cidx, True)
    cmask[:, K] = False                                           # as the corpus builds it: the padding cluster is unmasked by the encoder only
    G = Hn + K
    graph = torch.rand(B, G, G, generator=g) * (torch.rand(B, G, G, generator=g) < 0.3)
    graph = graph + torch.eye(G)
    graph = graph / graph.sum(dim=2, keepdim=True)
    return hist, cand, dout, hmask, cidx, cmask, graph.float()


def _state_of(enc):
    return {'user_encoder.' + k: v.detach().cpu().numpy() for k, v in enc.state_dict().items() if not k.startswith('news_encoder.')}


def _run_encoder(name, shape, p):
    """One forward + backward of the encoder on the first input seed whose float64 run keeps RELU_MARGIN; returns (got, exp, extras)."""
    import hip_masks
    B, N, Hn, K, D = shape
    for seed in range(100, 160):
        enc, cfg = _encoder(name, shape, p, seed)
        hist, cand, dout, hmask, cidx, cmask, graph = _enc_inputs(shape, seed)
        st = _state_of(enc)
        useed = hip_masks._user_seed(enc)
        if name == 'SUE_wo_GCN':
            keep = hip_masks.flat_keep(B * N * (K + 1) * D, p, useed + 2).view(B, N, K + 1, D).cpu()
            exp = R.sue_wo_gcn(hist, cand, cmask, cidx, st, keep=keep, p=p, dout=dout)
        else:
            kp = hip_masks.flat_keep(B * K * D, p, useed + 1).view(B, K, D).cpu()
            kg = {l: hip_masks.flat_keep(B * (Hn + K) * D, p / 2, useed + 10 + l).view(B, Hn + K, D).cpu() for l in range(cfg.gcn_layer_num - 1)}
            exp = R.sue_wo_hca(hist, graph, st, N, cfg, keep_proxy=kp, keep_gcn=kg, p=p, dout=dout)
        if exp['relu_margin'] >= RELU_MARGIN:
            break
    else:
        raise AssertionError('no seed keeps the relu margin')
    h, c = hist.cuda().requires_grad_(), cand.cuda().requires_grad_()
    cm = cmask.cuda()
    out = enc.encode_user(h, hmask.cuda(), graph.cuda(), cm, cidx.cuda(), c)
    out.backward(dout.cuda())
    torch.cuda.synchronize()
    got = {'user_rep': out, 'dhist': h.grad}
    if name == 'SUE_wo_GCN':
        got['dcand'] = c.grad
    else:
        assert c.grad is None                                     # SUE_wo_HCA never reads the candidates
        exp.pop('dcand', None)
    for k, q in enc.named_parameters():
        assert q.grad is not None, k
        got['grad/' + k] = q.grad
    return got, exp, dict(enc=enc, cmask_before=cmask, cmask_after=cm.cpu(), seed=seed, margin=exp['relu_margin'])


@pytest.mark.parametrize('p', [0.0, 0.2], ids=['dropout_off', 'dropout_on'])
@pytest.mark.parametrize('shape', ENC_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('name', ['SUE_wo_GCN', 'SUE_wo_HCA'])
def test_encoder_matches_the_float64_restatement(name, shape, p):
    got, exp, ex = _run_encoder(name, shape, p)
    exp = {k: v for k, v in exp.items() if torch.is_tensor(v) and k not in ('alpha', 'feat')}
    kb = 'grad/intraCluster_K.bias'
    if name == 'SUE_wo_GCN':
        assert float(got[kb].abs().max()) == 0.0 and tuple(got[kb].shape) == tuple(ex['enc'].intraCluster_K.bias.shape)     # exactly zero, not None
        assert float(exp.pop(kb).abs().max()) <= 1e-12 * float(exp['grad/intraCluster_Q.bias'].abs().max())
        after = ex['cmask_before'].clone()
        after[:, -1] = True
        assert torch.equal(ex['cmask_after'], after) and not bool(ex['cmask_before'][:, -1].any())     # the mask's last column is written in place
    else:
        assert torch.equal(ex['cmask_after'], ex['cmask_before'])                                       # bit-identical
    assert sorted(got) == sorted(list(exp) + ([kb] if name == 'SUE_wo_GCN' else []))
    _check(got, exp, '%s %s p=%g (seed %d, relu margin %.1e)' % (name, shape, p, ex['seed'], ex['margin']), grads=[k for k in exp if k != 'user_rep'])


def test_parameter_gradients_accumulate_reproducibly():
    """Two backward passes without zeroing add up (bit for bit twice the single pass), and a fresh run gives the same bits."""
    runs = []
    for reps in (1, 2, 1):
        enc, _ = _encoder('SUE_wo_GCN', ENC_SHAPES[0], 0.0, 7)
        hist, cand, dout, hmask, cidx, cmask, graph = _enc_inputs(ENC_SHAPES[0], 7)
        for _ in range(reps):
            out = enc.encode_user(hist.cuda(), hmask.cuda(), graph.cuda(), cmask.cuda(), cidx.cuda(), cand.cuda().requires_grad_())
            out.backward(dout.cuda())
        torch.cuda.synchronize()
        runs.append({k: q.grad.clone() for k, q in enc.named_parameters()})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[2][k]), k
        assert torch.equal(runs[1][k], 2 * runs[0][k]), k


# ------------------------------------------------------------------------------------------------ the shared stages
STAGE_SHAPE = (3, 2, 6, 3, 20)          # (B, N, Hn, K, D); two GCN layers, dropout on


def test_gcn_feature_stage_is_one_stage_in_sue_and_sue_wo_hca():
    """A SUE and a SUE_wo_HCA with the same proxy nodes, GCN weights and seed counter: SUE_wo_HCA's GCN feature is SUE's captured one bit for
    bit, and so are the GCN / proxy / history gradients of the stage's backward for the same d gfeat."""
    from nnr_amd import ops, user_encoders as UE
    sue, _ = _encoder('SUE', STAGE_SHAPE, 0.2, 11, layers=2)
    hca, _ = _encoder('SUE_wo_HCA', STAGE_SHAPE, 0.2, 11, layers=2)
    with torch.no_grad():
        hca.proxy_node_embedding.copy_(sue.proxy_node_embedding)
    hca.gcn.load_state_dict(sue.gcn.state_dict())
    hist, cand, dout, hmask, cidx, cmask, graph = (t.cuda() for t in _enc_inputs(STAGE_SHAPE, 11))
    UE.CAPTURE[0] = []
    try:
        sue.encode_user(hist, hmask, graph, cmask, cidx, cand)
    finally:
        (sv,), UE.CAPTURE[0] = UE.CAPTURE[0], None
    h = hist.clone().requires_grad_()
    gfeat = UE._SueGcnFeatureFn.apply(h, hca, graph)
    assert torch.equal(gfeat, sv['gfeat']) and sv['p'] == 0.2 and len(sv['gcn']['rs']) == 2
    dg = torch.randn(gfeat.shape, generator=torch.Generator().manual_seed(12)).cuda()
    gfeat.backward(dg)
    with ops.leaf_scope(dg.device) as leaf:
        dhist = UE.gcn_feature_bwd(sue, sv['gcn'], sv['graph'], dg, sv['p'], sv['seed'], leaf)
    torch.cuda.synchronize()
    assert torch.equal(dhist, h.grad)
    assert torch.equal(sue.proxy_node_embedding.grad, hca.proxy_node_embedding.grad) and float(sue.proxy_node_embedding.grad.abs().max()) > 0
    for (k, a), (_, b) in zip(sue.gcn.named_parameters(), hca.gcn.named_parameters()):
        assert torch.equal(a.grad, b.grad) and float(a.grad.abs().max()) > 0, k


@pytest.mark.parametrize('name,calls', [('SUE', 36), ('SUE_wo_GCN', 21), ('SUE_wo_HCA', 25)])
def test_launch_budget_of_one_forward_and_backward(name, calls):
    """C-ABI calls of one encode_user + backward (forward + backward: SUE 13 + 23, SUE_wo_GCN 8 + 13, SUE_wo_HCA 10 + 15), counted on the
    commit before the three encoders were built from shared stages: exact."""
    from nnr_amd import _lib
    enc, _ = _encoder(name, STAGE_SHAPE, 0.2, 11, layers=2)
    hist, cand, dout, hmask, cidx, cmask, graph = (t.cuda() for t in _enc_inputs(STAGE_SHAPE, 11))
    h, c = hist.requires_grad_(), cand.requires_grad_()
    torch.cuda.synchronize()
    c0 = _lib.CALLS[0]
    enc.encode_user(h, hmask, graph, cmask, cidx, c).backward(dout)
    torch.cuda.synchronize()
    assert _lib.CALLS[0] - c0 == calls


# ------------------------------------------------------------------------------------------------ model level
@pytest.mark.parametrize('tag', CASES)
def test_model_matches_reference_golden(tag):
    """The body of tests/test_hip_catt_gpu.py::test_model_matches_reference_golden, bars unchanged.  intraCluster_K.bias is left out of the
    gradient and post-step comparisons (the reference's gradient of it is rounding noise that Adam normalises); it must come
    through the steps unchanged instead."""
    from nnr_amd.trainer import Trainer
    from nnr_amd.model import negative_log_softmax
    case = GoldenCase(tag)
    model, cfg = build_model(case)
    trainer = Trainer(model, cfg)
    steps = int(case.meta['adam_steps'])
    KB = 'user_encoder.intraCluster_K.bias'
    rec = {}
    ne = model.news_encoder
    if hasattr(ne, 'forward_pair'):                   # Model.forward drives CNE through the lock-step pair entry
        orig_pair = ne.forward_pair

        def recording_pair(c, h):
            a, b = orig_pair(c, h)
            rec['reps'] = [a.detach().cpu().numpy(), b.detach().cpu().numpy()]
            return a, b
        ne.forward_pair = recording_pair
    else:
        ne.register_forward_hook(lambda m, i, o: rec.setdefault('reps', []).append(o.detach().cpu().numpy()))
    ue = model.user_encoder
    orig_enc = ue.encode_user

    def recording_enc(*a):
        o = orig_enc(*a)
        rec['user'] = o.detach().cpu().numpy()
        return o
    ue.encode_user = recording_enc
    kb0 = dict(model.named_parameters())[KB].detach().clone() if 'wo_GCN' in tag else None
    report = []
    for s in range(steps):
        batch = case.batch('cuda')
        trainer.flat.zero_grad()
        logits = model(*batch)
        loss = negative_log_softmax(logits)
        loss.backward()
        torch.cuda.synchronize()
        if s == 0:
            e = {k: float(np.abs(v - case.expect(n)).max()) for k, v, n in
                 (('cand_rep', rec['reps'][0], 'cand_rep'), ('hist_rep', rec['reps'][1], 'hist_rep'), ('user_rep', rec['user'], 'user_rep'))}
            report.append('stage max-abs-err: %s' % e)
            lg = logits.detach().cpu().numpy()
            err = float(np.abs(lg - case.expect('logits')).max())
            report.append('logits err %.3e  loss err %.3e' % (err, abs(float(loss) - float(case.expect('loss')))))
            print('\n'.join(report))
            assert max(e.values()) <= TIGHT * max(1.0, float(np.abs(case.expect('hist_rep')).max())), e
            assert err <= LOGIT_TOL and err <= TIGHT * max(1.0, float(np.abs(lg).max())), err
            assert abs(float(loss) - float(case.expect('loss'))) <= TIGHT
            # in-place input mutation is part of the reference's observable behaviour
            np.testing.assert_array_equal(batch[16].cpu().numpy(), case.expect('mutated_news_title_mask'))
            np.testing.assert_array_equal(batch[11].cpu().numpy(), case.expect('mutated_user_history_category_mask'))
            total = float(case.expect('grad_total_norm'))
            for k, p in model.named_parameters():
                if k.startswith('user_encoder.news_encoder.') or k == KB:
                    continue
                exp, act = case.expect_grad(k, p.grad)
                scale = max(1e-3, float(case.expect('gradnorm/' + k)), 0.05 * total)
                assert float(np.abs(act - exp).max()) <= 5e-5 * scale, 'grad ' + k
                nk = float(case.expect('gradnorm/' + k))
                if exp.size == p.numel() and nk > 1e-4 * total:
                    rel = float(np.linalg.norm((act - exp).astype(np.float64))) / nk
                    assert rel <= 1e-3, 'grad %s: relative L2 error %.3e' % (k, rel)
                gn = float(p.grad.double().norm())
                assert abs(gn - float(case.expect('gradnorm/' + k))) <= 5e-5 * scale, 'gradnorm ' + k
            assert abs(trainer.grad_total_norm() - total) <= 2e-5 * max(1.0, total)
            if kb0 is not None:
                assert float(dict(model.named_parameters())[KB].grad.abs().max()) == 0.0      # exactly zero (the reference's autograd leaves rounding noise)
        assert abs(float(loss) - float(case.expect('loss_step%d' % s))) <= 5e-5, 'loss at step %d' % s
        trainer.optimizer_step(1.0)
    torch.cuda.synchronize()
    lr = float(cfg.lr)
    for k, p in model.named_parameters():
        if k.startswith('user_encoder.news_encoder.'):
            continue
        if k == KB:
            assert torch.equal(p.detach(), kb0)                  # a zero gradient: Adam leaves it where it was
            continue
        exp, act = case.expect_param(steps, k, p)
        dlt = np.abs(act - exp)
        assert dlt.max(initial=0.0) <= steps * lr * 1.01 + 1e-4, 'param (hard bound) ' + k
        if float(case.expect('gradnorm/' + k)) >= 1e-2 * float(case.expect('grad_total_norm')):   # gradient well above the noise floor
            assert float(dlt.mean()) <= max(2e-5, 0.05 * steps * lr), 'param (mean deviation) ' + k
    # the trainer's own step takes the autograd path for these pairs and records no tape
    for _ in range(4):
        _, loss = trainer.train_step(case.batch('cuda'))
        assert trainer.last_path == 'autograd'
    assert not trainer.tapes and bool(torch.isfinite(loss))


@pytest.mark.parametrize('tag', ['tiny_CNN_SUE_wo_GCN', 'tiny_CNN_SUE_wo_HCA'])
def test_reference_state_dict_loads_strictly_and_scores_match(tag):
    """eval_fixture loads the reference's own state_dict with strict=True; evaluate.compute_scores on the cached path (CNN's representations
    are batch-independent) and in the reference's per-sample form, bar as tests/test_hip_catt_gpu.py."""
    from nnr_amd import evaluate as E
    z, model = eval_fixture(tag)
    model = model.cuda().train()
    dc = E.dev_corpus({k: z[k] for k in z.files}, 'cuda', int(z['category_num']))
    assert E.news_reps_cacheable(model)
    cached = E.compute_scores(model, dc, batch_size=8)                    # 'auto' -> cached
    st = dict(E.LAST_STATS)
    plain = E.compute_scores(model, dc, batch_size=8, cache=False)
    assert st['mode'] == 'cached' and E.LAST_STATS['mode'] == 'per-sample' and model.training
    for name, got in (('cached', cached), ('per-sample', plain)):
        err = float(np.abs(got.cpu().numpy() - z['scores']).max())
        print('%s %s scores max-abs-err %.3e' % (tag, name, err))
        assert err <= 2e-5, (name, err)
    ranks, _, mean = E.rank_metrics(cached, torch.from_numpy(z['labels']), z['sizes'])
    np.testing.assert_array_equal(ranks.cpu().numpy(), z['ranks'])
    np.testing.assert_allclose(mean.cpu().numpy(), z['metrics'], rtol=0, atol=1e-12)
