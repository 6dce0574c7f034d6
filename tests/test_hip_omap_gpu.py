"""The OMAP (Hi-Fi Ark) user encoder on the GPU: the kernels of csrc/omap.hip against the float64 restatement of the reference's
formulation (tests/omap_ref.py, pinned to the reference by tests/test_omap_host.py), their reproducibility, the observable quirks
(padded rows in the archives, users without history, masked_fill's blocked gradients), the regulariser, and the model / trainer /
plugin / evaluation / dropout-on paths against golden vectors captured from the reference's own code (tests/golden/*OMAP*.npz).
Bars as in tests/test_hip_catt_gpu.py, tests/test_hip_model_gpu.py and tests/test_hip_eval_gpu.py."""

import numpy as np
import pytest
import torch

from omap_ref import omap_form, regularizer, omap_user_rep, f64
from golden_io import GoldenCase, build_model, eval_fixture

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4
TIGHT = 2e-5
OMAP_CASES = ['tiny_CNE_OMAP_stable', 'tiny_CNN_OMAP', 'full_CNE_OMAP_g0p35_stable']
#         B, N, H, D, K
SHAPES = [(64, 5, 50, 900, 3), (2, 5, 50, 900, 3), (5, 1, 50, 500, 3), (1, 1, 1, 4, 1), (7, 4, 33, 30, 5), (3, 3, 6, 40, 3),
          (2, 3, 70, 130, 16), (4, 3, 6, 40, 3)]      # (B = 1, 4, 5: the weight gradient sums one partial row per user, four loads at a time)
SCALE = {900: 0.3, 500: 0.4, 130: 0.5, 40: 0.5, 30: 0.6, 24: 0.6, 13: 0.6, 4: 0.6}      # keeps the three softmaxes off saturation (see _expected's assertion)


def _inputs(B, N, H, D, K, masked, seed):
    """fp32 inputs.  Masks: sample 0 without history, sample 1 with a full one, the others ragged."""
    g = torch.Generator().manual_seed(seed)
    X, C = SCALE[D] * torch.randn(B, H, D, generator=g), SCALE[D] * torch.randn(B, N, D, generator=g)
    W = torch.randn(D, K, generator=g) / K ** 0.5
    dout = torch.randn(B, N, D, generator=g)
    mask = None
    if masked:
        lens = torch.randint(0, H + 1, (B,), generator=g)
        lens[0] = 0
        if B > 1:
            lens[1] = H
        mask = torch.arange(H).unsqueeze(0) < lens.unsqueeze(1)
    return X, C, W, dout, mask


def _expected(X, C, W, dout, mask):
    """The restatement's outputs and gradients.  So that the comparison cannot pass vacuously it asserts that the part of dX that flows
    through alpha is at least 1 % of max|dX| and that dW is not zero -- wherever those paths exist: with one history slot alpha is the
    constant 1, and with one head beta is the constant 1 and dW is identically zero (then the kernel's dW must be exactly zero too)."""
    x, c, w = (f64(t).requires_grad_() for t in (X, C, W))
    r = omap_form(x, c, w, mask)
    (r['out'] * f64(dout)).sum().backward()
    exp = dict(alpha=r['alpha'].detach(), beta=r['beta'].detach(), gamma=r['gamma'].detach(), out=r['out'].detach(), dX=x.grad, dC=c.grad, dW=w.grad)
    if X.shape[1] > 1:
        x2 = f64(X).requires_grad_()
        (omap_form(x2, f64(C), f64(W), mask, detach_alpha=True)['out'] * f64(dout)).sum().backward()
        share = float((x.grad - x2.grad).abs().max()) / float(x.grad.abs().max())
        print('share of dX through alpha: %.4f' % share)
        assert share >= 0.01, share
    if W.shape[1] > 1:
        assert float(w.grad.abs().max()) > 0
    return exp


def _run(X, C, W, dout, mask, dX0=None, hist_dev=None):
    from nnr_amd import ops
    B, H, D = X.shape
    N, K = C.shape[1], W.shape[1]
    dev = dict(device='cuda', dtype=torch.float32)
    x = X.cuda().contiguous() if hist_dev is None else hist_dev
    c, w, do = (t.cuda().contiguous() for t in (C, W, dout))
    m = None if mask is None else mask.cuda().contiguous()
    alpha, Y, beta = torch.empty((B, H, H), **dev), torch.empty((B, H, D), **dev), torch.empty((B, H, K), **dev)
    R, gamma, out = torch.empty((B, K, D), **dev), torch.empty((B, N, K), **dev), torch.empty((B, N, D), **dev)
    ops.omap_fwd(x, c, m, w, B, N, H, D, K, alpha, Y, beta, R, gamma, out)
    dX = torch.empty((B, H, D), **dev) if dX0 is None else dX0.cuda().clone()
    dC, dW = torch.empty((B, N, D), **dev), torch.zeros((D, K), **dev)
    ops.omap_bwd(x, c, m, w, alpha, Y, beta, R, gamma, do, B, N, H, D, K, dX, dC, dW, accumulate=dX0 is not None)
    torch.cuda.synchronize()
    return dict(alpha=alpha, beta=beta, gamma=gamma, out=out, dX=dX, dC=dC, dW=dW, R=R, Y=Y)


def _check(got, exp, tag):
    """The rule of tests/test_hip_catt_gpu.py::_check: TIGHT x max(1, max|expected|); the weight gradient relative to its own max."""
    report, worst = [], {}
    for k, e in exp.items():
        err = float((got[k].cpu().double() - e).abs().max())
        emax = float(e.abs().max())
        bar = TIGHT * (emax if k == 'dW' else max(1.0, emax))
        report.append('%s err %.3e (max|exp| %.3e, bar %.3e)' % (k, err, emax, bar))
        worst[k] = (err, bar)
    print(tag + ': ' + '; '.join(report))
    for k, (err, bar) in worst.items():
        assert err <= bar, (tag, k, err, bar)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('masked', [True, False], ids=['mask', 'nomask'])
def test_kernels_match_the_float64_restatement(shape, masked):
    inp = _inputs(*shape, masked, seed=sum(shape) + 7 * masked)
    _check(_run(*inp), _expected(*inp), '%s %s' % (shape, 'mask' if masked else 'nomask'))


def test_padded_rows_carry_uniform_beta_and_feed_the_archives():
    """Quirk 1: beta == 1/K exactly on a padded row, and its X row is part of R."""
    B, N, H, D, K = 3, 3, 6, 40, 3
    X, C, W, dout, _ = _inputs(B, N, H, D, K, False, seed=31)
    mask = torch.tensor([[1, 1, 1, 0, 0, 0], [1, 1, 1, 1, 1, 1], [1, 0, 1, 0, 1, 0]], dtype=torch.bool)
    a = _run(X, C, W, dout, mask)
    pad = ~mask
    assert bool((a['beta'].cpu()[pad] == np.float32(1.0) / np.float32(K)).all())
    X2 = X.clone()
    X2[0, 4] += 0.5                                           # a padded row of sample 0
    b = _run(X2, C, W, dout, mask)
    assert float((a['R'][0] - b['R'][0]).abs().max()) > 1e-2   # ... moves that sample's archives
    assert torch.equal(a['R'][1], b['R'][1])
    _check(b, _expected(X2, C, W, dout, mask), 'padded rows')


def test_a_user_without_history_attends_uniformly_and_blocks_the_score_gradient():
    """Quirks 2 and 3: alpha == 1/H over all slots; dS = 0 there (masked_fill), although the softmax-backward formula alone is not zero;
    db = 0 on padded rows."""
    B, N, H, D, K = 3, 3, 6, 40, 3
    X, C, W, dout, _ = _inputs(B, N, H, D, K, False, seed=37)
    mask = torch.tensor([[0] * 6, [1] * 6, [1, 1, 0, 0, 0, 0]], dtype=torch.bool)
    got = _run(X, C, W, dout, mask)
    assert bool((got['alpha'][0].cpu() == np.float32(1.0) / np.float32(H)).all())
    exp = _expected(X, C, W, dout, mask)
    _check(got, exp, 'no history')
    # the softmax-backward formula alone (same forward values, masked scores not blocked) gives sample 0 a visibly different dX: the
    # comparison above does pin dS = 0
    x = f64(X).requires_grad_()
    (omap_form(x, f64(C), f64(W), mask, unblocked=True)['out'] * f64(dout)).sum().backward()
    gap = float((x.grad[0] - exp['dX'][0]).abs().max())
    print('unblocked vs blocked dX of the user without history: %.3e (bar %.3e)' % (gap, TIGHT * max(1.0, float(exp['dX'].abs().max()))))
    assert gap > 100 * TIGHT * max(1.0, float(exp['dX'].abs().max()))


def test_kernel_accumulates_into_a_given_history_gradient():
    inp = _inputs(3, 3, 6, 40, 3, True, seed=5)
    base = torch.randn(3, 6, 40, generator=torch.Generator().manual_seed(9))
    exp = _expected(*inp)
    exp['dX'] = exp['dX'] + base.double()
    _check(_run(*inp, dX0=base), exp, 'accumulate')


def test_row_strided_history():
    """hist as a [B, H, D] view of rows that are 2 D wide (ldf = 2 D)."""
    B, N, H, D, K = 3, 2, 7, 24, 3
    X, C, W, dout, mask = _inputs(B, N, H, D, K, True, seed=13)
    wide = torch.randn(B, H, 2 * D, device='cuda')
    view = wide[:, :, :D]
    view.copy_(X)
    assert view.stride(1) == 2 * D
    _check(_run(X, C, W, dout, mask, hist_dev=view), _expected(X, C, W, dout, mask), 'row stride')


def test_unaligned_rows_and_odd_widths():
    """D % 4 != 0, and a history tensor that starts 4 bytes off a 16-byte boundary."""
    B, N, H, D, K = 2, 2, 5, 13, 2
    X, C, W, dout, mask = _inputs(B, N, H, D, K, True, seed=11)
    store = torch.zeros(B * H * D + 1, device='cuda')
    xo = store[1:].view(B, H, D)
    xo.copy_(X)
    assert xo.data_ptr() % 16 == 4
    _check(_run(X, C, W, dout, mask, hist_dev=xo), _expected(X, C, W, dout, mask), 'unaligned')


def test_unsupported_sizes_are_refused_on_the_host():
    from nnr_amd import _lib
    L = _lib.lib()
    assert L.nnr_omap_ws_floats(2, 5, 50, 900, 17) == -3 and L.nnr_omap_ws_floats(2, 5, 97, 900, 3) == -3      # NNR_ERR_UNSUPPORTED
    assert L.nnr_omap_ws_floats(2, 5, 0, 900, 3) == -1 and L.nnr_omap_ws_floats(2, 5, 96, 900, 16) > 0


def test_kernels_are_bit_reproducible():
    inp = _inputs(64, 5, 50, 900, 3, True, seed=21)
    a, b = _run(*inp), _run(*inp)
    for k in ('alpha', 'beta', 'gamma', 'out', 'dX', 'dC', 'dW'):
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ the regulariser
def _reg(W, coef, gup=1.0):
    from nnr_amd import ops
    w = W.cuda().contiguous()
    K = w.shape[1]
    off, loss = torch.empty(K * K + 1, device='cuda'), torch.empty((), device='cuda')
    ops.omap_reg_fwd(w, coef, off, loss)
    dW = torch.zeros_like(w)
    ops.omap_reg_bwd(w, off, torch.tensor(gup, device='cuda'), coef, dW)
    torch.cuda.synchronize()
    return loss, dW


@pytest.mark.parametrize('shape', [(900, 3), (36, 3), (500, 8)], ids=lambda s: 'x'.join(map(str, s)))
def test_regulariser_matches_float64(shape):
    W = torch.randn(*shape, generator=torch.Generator().manual_seed(shape[0])) / shape[1] ** 0.5
    w = f64(W).requires_grad_()
    e = regularizer(w, 0.1)
    e.backward()
    loss, dW = _reg(W, 0.1)
    lerr, gerr = abs(float(loss) - float(e)), float((dW.cpu().double() - w.grad).abs().max())
    print('regulariser %s: loss %.6f err %.3e, dW err %.3e (max %.3e)' % (shape, float(e), lerr, gerr, float(w.grad.abs().max())))
    assert lerr <= TIGHT * max(1.0, abs(float(e))) and gerr <= TIGHT * float(w.grad.abs().max())
    _, dW3 = _reg(W, 0.1, gup=-2.5)                              # the upstream gradient scales it
    assert float((dW3.cpu().double() + 2.5 * w.grad).abs().max()) <= TIGHT * 2.5 * float(w.grad.abs().max())


def test_regulariser_is_exactly_zero_at_orthogonal_columns():
    W = torch.zeros(36, 3)
    W[2, 0], W[7, 1], W[30, 2] = 1.0, -2.0, 0.5                 # distinct unit directions: W^T W is diagonal exactly
    loss, dW = _reg(W, 0.1)
    assert float(loss) == 0.0 and float(dW.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the model
def _trainer_loss(model, logits):
    """The loss as Trainer._train_step forms it (trainer.py:109-114 of the reference)."""
    from nnr_amd.model import negative_log_softmax
    loss = negative_log_softmax(logits)
    if model.news_encoder.auxiliary_loss is not None:
        loss = loss + model.news_encoder.auxiliary_loss.mean()
    if model.user_encoder.auxiliary_loss is not None:
        loss = loss + model.user_encoder.auxiliary_loss.mean()
    return loss


@pytest.mark.parametrize('tag', OMAP_CASES)
def test_model_matches_reference_golden(tag):
    """The body of tests/test_hip_model_gpu.py::test_model_matches_reference_golden, bars unchanged; the loss is the trainer's."""
    from nnr_amd.trainer import Trainer
    from nnr_amd.model import negative_log_softmax
    case = GoldenCase(tag)
    model, cfg = build_model(case)
    trainer = Trainer(model, cfg)
    steps = int(case.meta['adam_steps'])
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
    assert ue.auxiliary_loss is None
    orig_enc = ue.encode_user

    def recording_enc(*a):
        o = orig_enc(*a)
        rec['user'] = o.detach().cpu().numpy()
        return o
    ue.encode_user = recording_enc
    report = []
    for s in range(steps):
        batch = case.batch('cuda')
        trainer.flat.zero_grad()
        logits = model(*batch)
        loss = _trainer_loss(model, logits)
        loss.backward()
        torch.cuda.synchronize()
        if s == 0:
            e = {k: float(np.abs(v - case.expect(n)).max()) for k, v, n in
                 (('cand_rep', rec['reps'][0], 'cand_rep'), ('hist_rep', rec['reps'][1], 'hist_rep'), ('user_rep', rec['user'], 'user_rep'))}
            report.append('stage max-abs-err: %s' % e)
            lg = logits.detach().cpu().numpy()
            err = float(np.abs(lg - case.expect('logits')).max())
            report.append('logits err %.3e  loss err %.3e  auxiliary err %.3e' % (err, abs(float(loss) - float(case.expect('loss'))),
                                                                                  abs(float(ue.auxiliary_loss) - float(case.expect('auxiliary_loss')))))
            print('\n'.join(report))
            assert max(e.values()) <= TIGHT * max(1.0, float(np.abs(case.expect('hist_rep')).max())), e
            assert err <= LOGIT_TOL and err <= TIGHT * max(1.0, float(np.abs(lg).max())), err
            assert abs(float(loss) - float(case.expect('loss'))) <= TIGHT
            assert ue.auxiliary_loss.dim() == 0 and abs(float(ue.auxiliary_loss) - float(case.expect('auxiliary_loss'))) <= TIGHT
            # in-place input mutation is part of the reference's observable behaviour
            np.testing.assert_array_equal(batch[16].cpu().numpy(), case.expect('mutated_news_title_mask'))
            np.testing.assert_array_equal(batch[11].cpu().numpy(), case.expect('mutated_user_history_category_mask'))
            total = float(case.expect('grad_total_norm'))
            for k, p in model.named_parameters():
                if k.startswith('user_encoder.news_encoder.'):
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
        assert abs(float(loss) - float(case.expect('loss_step%d' % s))) <= 5e-5, 'loss at step %d' % s
        trainer.optimizer_step(1.0)
    torch.cuda.synchronize()
    lr = float(cfg.lr)
    for k, p in model.named_parameters():
        if k.startswith('user_encoder.news_encoder.'):
            continue
        exp, act = case.expect_param(steps, k, p)
        dlt = np.abs(act - exp)
        assert dlt.max(initial=0.0) <= steps * lr * 1.01 + 1e-4, 'param (hard bound) ' + k
        if float(case.expect('gradnorm/' + k)) >= 1e-2 * float(case.expect('grad_total_norm')):   # gradient well above the noise floor
            assert float(dlt.mean()) <= max(2e-5, 0.05 * steps * lr), 'param (mean deviation) ' + k
    # the trainer's own step takes the autograd path for this pair, records no tape, and returns click loss + auxiliary term
    ue.encode_user = orig_enc
    for i in range(4):
        logits, loss = trainer.train_step(case.batch('cuda'))
        assert trainer.last_path == 'autograd'
        if i == 0:
            click = float(negative_log_softmax(logits))
            aux = float(ue.auxiliary_loss)
            print('trainer step: loss %.6f = click %.6f + auxiliary %.6f' % (float(loss), click, aux))
            assert aux > 0.01 and abs(float(loss) - (click + aux)) <= 1e-6 * max(1.0, abs(float(loss)))
    assert not trainer.tapes and bool(torch.isfinite(loss))


@pytest.mark.parametrize('tag', ['tiny_CNE_OMAP_stable', 'full_CNE_OMAP_g0p35_stable'])
def test_plugin_calls_equal_lockstep_path(tag):
    case = GoldenCase(tag)
    model, cfg = build_model(case)
    b = case.batch('cuda')
    logits = model(*b).detach()
    b = case.batch('cuda')
    (uid, ucat, usub, utt, utm, ute, uct, ucm, uce, uhm, ug, ucmask, ucidx, ncat, nsub, ntt, ntm, nte, nct, ncm, nce) = b
    cand = model.news_encoder(ntt, ntm, nte, nct, ncm, nce, ncat, nsub, None)
    user = model.user_encoder(utt, utm, ute, uct, ucm, uce, ucat, usub, uhm, ug, ucmask, ucidx, None, cand)
    assert tuple(user.shape) == tuple(cand.shape)
    plug = (user * cand).sum(dim=2)
    assert float((plug - logits).abs().max()) <= 1e-6


def test_eval_mode_leaves_the_auxiliary_loss_untouched():
    case = GoldenCase('tiny_CNN_OMAP')
    model, cfg = build_model(case)
    ue = model.user_encoder
    model.eval()
    with torch.no_grad():
        model(*case.batch('cuda'))
    assert ue.auxiliary_loss is None                          # never set in eval mode
    model.train()
    model(*case.batch('cuda'))
    kept = ue.auxiliary_loss
    assert kept is not None and kept.dim() == 0
    model.eval()
    with torch.no_grad():
        model(*case.batch('cuda'))
    assert ue.auxiliary_loss is kept


# ------------------------------------------------------------------------------------------------ evaluation
def _eval_model(tag):
    z, model = eval_fixture(tag)
    return z, model.cuda().train()


@pytest.mark.parametrize('tag', ['tiny_CNN_OMAP', 'tiny_CNE_OMAP_stable'])
@pytest.mark.parametrize('graph', ['build', 'table'])
def test_compute_scores_and_metrics_match_reference(tag, graph):
    from nnr_amd import evaluate as E
    z, model = _eval_model(tag)
    dc = E.dev_corpus({k: z[k] for k in z.files}, 'cuda', int(z['category_num']), graph=graph)
    scores = E.compute_scores(model, dc, batch_size=8, cache=False)             # the reference's per-sample form
    assert model.training and E.LAST_STATS['mode'] == 'per-sample'
    got = scores.cpu().numpy()
    err = float(np.abs(got - z['scores']).max())
    print('%s scores max-abs-err %.3e' % (tag, err))
    assert err <= 2e-5, err
    ranks, per, mean = E.rank_metrics(scores, torch.from_numpy(z['labels']), z['sizes'])
    gaps = []
    o = 0
    for n in z['sizes']:
        s = np.sort(z['scores'][o:o + n]); gaps.append(np.diff(s).min() if n > 1 else 1.0); o += n
    assert min(gaps) > 1e-3                                                       # (asserted by the generator: the rank comparison is made)
    np.testing.assert_array_equal(ranks.cpu().numpy(), z['ranks'])
    np.testing.assert_allclose(mean.cpu().numpy(), z['metrics'], rtol=0, atol=1e-12)


def test_cached_news_representations_give_the_reference_scores():
    from nnr_amd import evaluate as E
    z, model = _eval_model('tiny_CNN_OMAP')
    dc = E.dev_corpus({k: z[k] for k in z.files}, 'cuda', int(z['category_num']))
    assert E.news_reps_cacheable(model)
    cached = E.compute_scores(model, dc, batch_size=8)                    # 'auto' -> cached
    st = dict(E.LAST_STATS)
    plain = E.compute_scores(model, dc, batch_size=8, cache=False)
    assert st['mode'] == 'cached' and E.LAST_STATS['mode'] == 'per-sample' and model.training
    assert float((cached - plain).abs().max()) <= 2e-6
    assert float(np.abs(cached.cpu().numpy() - z['scores']).max()) <= 2e-5
    assert st['encoder_rows'] * 2 <= st['per_sample_rows']
    ranks, _, mean = E.rank_metrics(cached, torch.from_numpy(z['labels']), z['sizes'])
    np.testing.assert_array_equal(ranks.cpu().numpy(), z['ranks'])
    np.testing.assert_allclose(mean.cpu().numpy(), z['metrics'], rtol=0, atol=1e-12)


def test_cne_omap_still_refuses_caching():
    """CNE + OMAP scores per sample, through the inference path without the redundant PAD slots: OMAP reads the padded rows (quirk 1), so
    this pins that their de-duplicated representation is the one the reference computed."""
    from nnr_amd import evaluate as E
    z, model = _eval_model('tiny_CNE_OMAP_stable')
    assert not E.news_reps_cacheable(model)
    dc = E.dev_corpus({k: z[k] for k in z.files}, 'cuda', int(z['category_num']))
    scores = E.compute_scores(model, dc, batch_size=8)                    # 'auto' -> per-sample
    assert E.LAST_STATS['mode'] == 'per-sample'
    assert float(np.abs(scores.cpu().numpy() - z['scores']).max()) <= 2e-5


def test_dropout_on_training_steps_feed_omap_what_the_news_encoder_produced():
    """CNE + OMAP at the 200k defaults (dropout 0.2), batch 8: two steps on the same batch draw different masks, and the OMAP stage
    (which has no dropout site of its own) turns the recorded history / candidate representations of that very run into the
    restatement's user representation."""
    from nnr_amd.config import make_config
    from nnr_amd.model import Model
    from nnr_amd.synth import SynthSpec, SynthCorpus, to_torch
    from nnr_amd.trainer import Trainer
    cfg = make_config(['--news_encoder=CNE', '--user_encoder=OMAP', '--batch_size=8'], corpus_sizes=dict(vocabulary_size=2000))
    assert cfg.dropout_rate == 0.2 and cfg.OMAP_head_num == 3 and cfg.HiFi_Ark_regularizer_coefficient == 0.1
    torch.manual_seed(0)
    model = Model(cfg)
    model.initialize()
    model = model.cuda().train()
    trainer = Trainer(model, cfg)
    batch = SynthCorpus(SynthSpec(vocabulary_size=cfg.vocabulary_size, news_pool=400, seed=3)).batch(8, np.random.default_rng(5))
    rec = []
    ne, ue = model.news_encoder, model.user_encoder
    orig_pair, orig_enc = ne.forward_pair, ue.encode_user

    def recording_pair(c, h):
        a, b = orig_pair(c, h)
        rec.append(dict(cand=a.detach().clone(), hist=b.detach().clone()))
        return a, b

    def recording_enc(*a):
        o = orig_enc(*a)
        rec[-1].update(user=o.detach().clone(), mask=a[1].clone(), W=ue.W.detach().clone())
        return o
    ne.forward_pair, ue.encode_user = recording_pair, recording_enc
    outs = []
    for _ in range(3):
        logits, loss = trainer.train_step(to_torch(batch, 'cuda'))
        torch.cuda.synchronize()
        assert trainer.last_path == 'autograd' and bool(torch.isfinite(loss))
        outs.append(logits.clone())
    assert float((outs[0] - outs[1]).abs().max()) > 1e-4                  # the second step drew other dropout masks
    for r in rec:
        exp = omap_user_rep(r['hist'], r['cand'], r['mask'], r['W'])
        err = float((r['user'].cpu().double() - exp).abs().max())
        print('OMAP stage vs restatement %.3e (max|exp| %.3e)' % (err, float(exp.abs().max())))
        assert err <= TIGHT * max(1.0, float(exp.abs().max()))
