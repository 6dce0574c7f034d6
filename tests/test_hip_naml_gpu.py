"""GPU tests of the single-view NAML news encoders: the view-pool kernels of csrc/naml.hip op by op against float64 (tests/naml_ref.py), and
the model against the reference's own results (tests/golden/*NAML*.npz) on both matrix paths, with dropout on, through evaluation, and
twice for bit equality.  Bars: those of tests/test_hip_kcnn_gpu.py -- 1e-4 of each tensor's scale (max |expected|), every element."""

import numpy as np
import pytest
import torch

from golden_io import GoldenCase, build_model, eval_fixture
import naml_ref
from naml_ref import f64

pytestmark = pytest.mark.gpu

BAR = 1e-4                 # the project's headline bar: of each tensor's own scale (max |expected|), every element
LOGIT_TOL = 1e-4
TIGHT = 2e-5
TINY = ['tiny_NAML_Title_ATT', 'tiny_NAML_Content_ATT', 'tiny_NAML_Content_CATT']
FULL = 'full_NAML_Title_ATT_g1p0'
# CATT's score bias shifts every history slot's score alike: the softmax does not see it and its gradient is zero on paper.  What fp32
# leaves there is the rounding of the terms that cancel, which are the terms of affine2.weight's gradient: that tensor's scale stands in
# (tests/test_hip_kcnn_gpu.py).
ZERO_ON_PAPER = {'user_encoder.affine2.bias': 'user_encoder.affine2.weight'}
# Adam divides a gradient by its own magnitude.  An element whose gradient is zero on paper (a relu unit of CATT that is dead or active for
# every history slot; CATT's score bias) holds fp32 rounding noise in the reference's own run too, and Adam turns that noise into steps of
# +-lr in a direction no implementation can reproduce.  Elements whose gradient in the reference's FLOAT64 run is below this fraction of the
# tensor's largest are therefore held to Adam's largest possible travel, steps x lr, not to the bar; every other element is held to the bar.
# 1e-6: an fp32 sum of terms of the tensor's scale carries a few 2^-24 = 6e-8 of it; sixteen times that.
NOISE_FLOOR = 1e-6


def dev():
    return torch.device('cuda')


# ------------------------------------------------------------------------------------------------ the view pool, op level
def _pool_case(n, C, Vt, pattern, big):
    """Inputs of one view-pool call.  pattern 'unused': table row 1 of A and the last row of B are named by no news; 'one': every news names
    row 2 of A and row 0 of B.  big: the scores are +-80 (whole views at weight exactly 0 or 1 in fp32)."""
    g = torch.Generator().manual_seed(100 * n + C + 7 * Vt + (3 if big else 0))
    Ra, Rb = 4, 6
    texts = [torch.randn(n, C, generator=g) for _ in range(Vt)]
    rowsA, rowsB = torch.relu(torch.randn(Ra, C, generator=g)), torch.relu(torch.randn(Rb, C, generator=g))
    draw = (lambda m: 80.0 * (2.0 * torch.randint(0, 2, (m,), generator=g).float() - 1.0)) if big else (lambda m: 2.0 * torch.randn(m, generator=g))
    scores = [draw(n) for _ in range(Vt)]
    scoreA, scoreB = draw(Ra), draw(Rb)
    if pattern == 'one':
        ia, ib = torch.full((n,), 2, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)
    else:
        ia = torch.tensor([0, 2, 3, 3, 0, 2, 2, 3, 0, 0][:n] if n <= 10 else [(0, 2, 3)[i % 3] for i in range(n)], dtype=torch.int32)
        ib = torch.randint(0, Rb - 1, (n,), generator=g, dtype=torch.int32)
    dout = torch.randn(n, C, generator=g)
    return texts, scores, rowsA, scoreA, ia, rowsB, scoreB, ib, dout


def _run_pool(case):
    from nnr_amd import ops
    texts, scores, rowsA, scoreA, ia, rowsB, scoreB, ib, dout = (([t.to(dev()) for t in x] if isinstance(x, list) else x.to(dev())) for x in case)
    Vt, (n, C) = len(texts), texts[0].shape
    nan = lambda *s: torch.full(s, float('nan'), device=dev())
    alpha, out = nan(n, Vt + 2), nan(n, C)
    ops.view_pool_fwd(texts, scores, rowsA, scoreA, ia, rowsB, scoreB, ib, alpha, out)
    grads = []
    for _ in range(2):
        dtexts, dts = [nan(n, C) for _ in range(Vt)], [nan(n) for _ in range(Vt)]
        drA, dsA, drB, dsB = nan(*rowsA.shape), nan(rowsA.shape[0]), nan(*rowsB.shape), nan(rowsB.shape[0])
        ops.view_pool_bwd(dout, texts, rowsA, ia, rowsB, ib, alpha, dtexts, dts, drA, dsA, drB, dsB)
        ops.join_extra_streams()
        torch.cuda.synchronize()
        grads.append([t.cpu() for t in dtexts + dts + [drA, dsA, drB, dsB]])
    return alpha.cpu(), out.cpu(), grads


@pytest.mark.parametrize('big', [False, True], ids=['scores', 'scores80'])
@pytest.mark.parametrize('pattern', ['unused', 'one'])
@pytest.mark.parametrize('Vt', [1, 2])
@pytest.mark.parametrize('shape', [(5, 7), (5, 400), (9, 70)], ids=lambda s: '%dx%d' % s)
def test_view_pool_forward_and_backward(shape, Vt, pattern, big):
    """alpha, out and the eight gradients (every element written: NaN prefill) within 1e-4 of each tensor's scale of float64 autograd over
    naml_ref.view_pool; a table row no news names gets exactly zero; scores of +-80 leave weights of exactly 0; the backward run twice
    gives the same bits."""
    n, C = shape
    case = _pool_case(n, C, Vt, pattern, big)
    texts, scores, rowsA, scoreA, ia, rowsB, scoreB, ib, dout = case
    alpha, out, grads = _run_pool(case)
    leaves = [f64(t).requires_grad_() for t in texts + scores + [rowsA, scoreA, rowsB, scoreB]]
    lt, ls = leaves[:Vt], leaves[Vt:2 * Vt]
    eout, ealpha = naml_ref.view_pool(lt, ls, leaves[2 * Vt], leaves[2 * Vt + 1], ia, leaves[2 * Vt + 2], leaves[2 * Vt + 3], ib)
    (eout * dout.double()).sum().backward()
    assert float((alpha.double() - ealpha.detach()).abs().max()) <= BAR and float((alpha.sum(dim=1) - 1).abs().max()) <= 1e-6
    assert float((out.double() - eout.detach()).abs().max()) <= BAR * float(eout.detach().abs().max())
    if big:                  # exp(-160) is zero in fp32 and 3e-70 in float64
        assert torch.equal(alpha == 0, ealpha.detach() < 1e-30) and bool(((alpha == 0) | (alpha > 0.2)).all())
    exp = [l.grad for l in lt + ls + leaves[2 * Vt:]]
    names = ['dt%d' % v for v in range(Vt)] + ['dts%d' % v for v in range(Vt)] + ['drowsA', 'dscoreA', 'drowsB', 'dscoreB']
    for name, got, e in zip(names, grads[0], exp):
        assert bool(torch.isfinite(got).all()), name
        scale = float(e.abs().max())
        err = float((got.double() - e).abs().max())
        print('%s %dx%d Vt%d %s: err %.2e of scale %.2e' % (name, n, C, Vt, pattern, err, scale))
        assert err <= BAR * max(scale, 1e-30) or (scale == 0 and err == 0), (name, err, scale)
    unusedA = [r for r in range(rowsA.shape[0]) if r not in ia.tolist()]
    assert unusedA and all(float(grads[0][2 * Vt][r].abs().max()) == 0.0 and float(grads[0][2 * Vt + 1][r]) == 0.0 for r in unusedA)
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def test_view_pool_over_many_news_and_long_segments():
    """n = 1000 news (250 workgroups of the per-news kernels; every wave of the table reduction scans four blocks of 64 ids, the last one
    partial, and walks ~21 matches per block: several rounds of eight rows), C = 130 (three column chunks, the last one partial)."""
    n, C, Vt = 1000, 130, 1
    case = _pool_case(n, C, Vt, 'unused', False)
    texts, scores, rowsA, scoreA, ia, rowsB, scoreB, ib, dout = case
    alpha, out, grads = _run_pool(case)
    leaves = [f64(t).requires_grad_() for t in texts + scores + [rowsA, scoreA, rowsB, scoreB]]
    eout, _ = naml_ref.view_pool(leaves[:1], leaves[1:2], leaves[2], leaves[3], ia, leaves[4], leaves[5], ib)
    (eout * dout.double()).sum().backward()
    assert float((out.double() - eout.detach()).abs().max()) <= BAR * float(eout.detach().abs().max())
    for got, leaf in zip(grads[0], leaves):
        e = leaf.grad
        assert float((got.double() - e).abs().max()) <= BAR * float(e.abs().max())
    for a, b in zip(*grads):
        assert torch.equal(a, b)


@pytest.mark.parametrize('dims', [(0, 4, 1), (4, 0, 1), (4, 4, 0), (4, 4, 3)], ids=lambda d: 'n%d_C%d_Vt%d' % d)
def test_unsupported_sizes_are_refused(dims):
    """A non-positive dimension and Vt outside 1..2 raise (code -3) instead of launching."""
    from nnr_amd import ops, _lib
    n, C, Vt = dims
    d = dev()
    z = lambda *s: torch.zeros(*s, device=d)
    texts, scores = [z(max(n, 1), max(C, 1)) for _ in range(Vt)], [z(max(n, 1)) for _ in range(Vt)]
    rows, sc, ids = z(3, max(C, 1)), z(3), torch.zeros(max(n, 1), device=d, dtype=torch.int32)
    lib = _lib.lib()
    p = lambda t: t.data_ptr()
    t0 = texts[0] if texts else rows
    rc = lib.nnr_view_pool_fwd(p(t0), p(sc), p(t0), p(sc), Vt, p(rows), p(sc), p(ids), 3, p(rows), p(sc), p(ids), 3, n, C, p(z(8, 8)), p(z(8, 8)), None)
    assert rc == _lib.NNR_ERR_UNSUPPORTED == -3
    if Vt in (1, 2):
        with pytest.raises(_lib.NnrHipError, match='unsupported size'):
            ops.view_pool_fwd([t[:n] for t in texts], scores, rows, sc, ids, rows, sc, ids, z(n, Vt + 2), z(n, C))


# ------------------------------------------------------------------------------------------------ the padded-row convolution
# An fp32 pre-activation is a sum of K = k E <= 60 products plus the bias: its error is at most (K + 1) 2^-24 times the sum of the terms'
# magnitudes, which stays below the tensor's scale: 4e-6 of it.  A pre-activation further than that from zero has the float64 sign.
RELU_MARGIN = 4e-6
CONV_SHAPES = [(3, 5, 12, 7, 3), (3, 5, 10, 6, 3), (2, 5, 12, 8, 5), (2, 3, 12, 5, 3), (3, 5, 12, 7, 1), (2, 7, 10, 9, 5), (4, 9, 16, 130, 3)]      # (n, L, E, C, k)


def _conv_inputs(n, L, E, C, k, seed):
    g = torch.Generator().manual_seed(seed)
    V = 23
    table = torch.randn(V, E, generator=g)
    text = torch.randint(0, V, (n, L), generator=g, dtype=torch.int32)
    text[0, -1] = 0
    weight, bias = torch.randn(C, E, k, generator=g) / (E * k) ** 0.5, 0.3 * torch.randn(C, generator=g)
    dy = torch.randn(n * L, C, generator=g)
    return table, text, weight, bias, dy


@pytest.mark.parametrize('p', [0.0, 0.5], ids=['p0', 'p05'])
@pytest.mark.parametrize('shape', CONV_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_conv_image_kernels(shape, p):
    """Forward image: every element written (NaN prefill), halo rows exactly zero, the word rows bit-equal to nnr_embed_gather's for the same
    p and seed (so the keep-mask is keyed on the compact rows).  dz: every element written, exactly zero in the k - 1 leading rows and at
    every row t >= L, (y > 0 ? dy : 0) bit for bit at the live rows.  Un-pad: dx bit-equal to the mask times the image's word rows; NaN in
    the halo rows of dXp never reaches it.  Shapes: E = 12 (16-byte path) and E = 10 (scalar path), L = k, k = 1 (no halo), 3 and 5, and
    one with more than one workgroup per kernel and C over one column block."""
    from nnr_amd import ops
    n, L, E, C, k = shape
    pad, Lp, lead = (k - 1) // 2, L + k - 1, k - 1
    table, text, weight, bias, dy = _conv_inputs(n, L, E, C, k, 11 + E + k)
    d = dev()
    seed = 77
    Xp = torch.full((n * Lp, E), float('nan'), device=d)
    ops.conv1d_image_fwd(table.to(d), text.reshape(-1).to(d), n, L, k, p, seed, Xp)
    X = Xp.cpu().view(n, Lp, E)
    assert bool((X[:, :pad] == 0).all()) and bool((X[:, pad + L:] == 0).all()) and X[:, pad + L:].shape[1] == k - 1 - pad
    if E % 4 == 0:
        rows = ops.embed_gather(table.to(d), text.reshape(-1).to(d), p, seed).cpu().view(n, L, E)
        keep = rows != 0 if p > 0 else torch.ones(n, L, E, dtype=torch.bool)
    else:                      # (nnr_embed_gather carries rows of a multiple of 4 floats: the flat mask of nnr_dropout is the same function)
        from hip_masks import flat_keep
        keep = flat_keep(n * L * E, p, seed).view(n, L, E).cpu()
        rows = torch.where(keep, table[text.long()] * (1.0 / (1.0 - p) if p > 0 else 1.0), torch.zeros(()))
    assert torch.equal(X[:, pad:pad + L], rows)
    if p > 0:
        assert 0.3 < float((X[:, pad:pad + L] != 0).float().mean()) < 0.7
    y = torch.randn(n * L, C, generator=torch.Generator().manual_seed(5))
    dz = torch.full((lead + n * Lp, C), float('nan'), device=d)
    ops.conv1d_dz_pad(dy.to(d), y.to(d), n, L, k, dz)
    got = dz.cpu()
    assert bool((got[:lead] == 0).all())
    body = got[lead:].view(n, Lp, C)
    assert bool((body[:, L:] == 0).all()) and torch.equal(body[:, :L].reshape(n * L, C), torch.where(y > 0, dy, torch.zeros(())))
    dX = torch.randn(n, Lp, E, generator=torch.Generator().manual_seed(6))
    halo = torch.ones(Lp, dtype=torch.bool)
    halo[pad:pad + L] = False
    dX[:, halo] = float('nan')
    dx = torch.full((n * L, E), float('nan'), device=d)
    ops.conv1d_image_bwd(dX.reshape(n * Lp, E).to(d), n, L, k, p, seed, dx)
    exp = torch.where(keep, dX[:, pad:pad + L] * (1.0 / (1.0 - p) if p > 0 else 1.0), torch.zeros(()))
    assert torch.equal(dx.cpu().view(n, L, E), exp)


@pytest.mark.parametrize('p', [0.0, 0.5], ids=['p0', 'p05'])
@pytest.mark.parametrize('shape', CONV_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_conv_as_one_product_matches_float64(shape, p):
    """functional.Conv1dImageFn, forward and backward, against float64 autograd over naml_ref.conv_rows fed the kernels' keep-mask: y (every
    compact row written, no junk row t >= L of the image in it), the weight, bias and table gradients within 1e-4 of each tensor's scale.
    The case's relu margin is asserted first (RELU_MARGIN), so no sign flip is excused."""
    from nnr_amd import ops, functional as Fn
    from hip_masks import flat_keep
    n, L, E, C, k = shape
    table, text, weight, bias, dy = _conv_inputs(n, L, E, C, k, 11 + E + k)
    d = dev()
    seed = 91
    conv = torch.nn.Conv1d(E, C, k, padding=(k - 1) // 2)
    with torch.no_grad():
        conv.weight.copy_(weight)
        conv.bias.copy_(bias)
    conv = conv.to(d)
    tab = torch.nn.Parameter(table.to(d))
    keep = flat_keep(n * L * E, p, seed).view(n, L, E).cpu()
    t64, w64, b64 = f64(table).requires_grad_(), f64(weight).requires_grad_(), f64(bias).requires_grad_()
    x = t64[text.long()] * keep.double() / (1.0 - p)
    z = naml_ref.conv_rows(x, w64, b64)
    margin = float(z.detach().abs().min() / z.detach().abs().max())
    y64 = torch.relu(z).reshape(n * L, C)
    y64.backward(dy.double())
    y = Fn.Conv1dImageFn.apply(tab, text.to(d), conv, n, L, p, seed, True)
    y.backward(dy.to(d))
    ops.join_extra_streams()
    torch.cuda.synchronize()
    print('conv %s p %.1f: smallest |pre-activation| %.1e of the scale' % (shape, p, margin))
    assert margin >= RELU_MARGIN, (shape, p, margin)
    for name, got, exp in (('y', y.detach(), y64.detach()), ('dweight', conv.weight.grad, w64.grad), ('dbias', conv.bias.grad, b64.grad), ('dtable', tab.grad, t64.grad)):
        err, s = float((got.cpu().double() - exp).abs().max()), float(exp.abs().max())
        print('  %s err %.2e of scale %.2e' % (name, err, s))
        assert bool(torch.isfinite(got).all()) and err <= BAR * s, (name, err, s)


@pytest.mark.parametrize('dims', [(0, 5, 8, 3), (2, 0, 8, 3), (2, 5, 0, 3), (2, 5, 8, 2), (2, 5, 8, 4), (2, 9, 8, 9), (2, 5, 8, 0)], ids=lambda d: 'n%d_L%d_E%d_k%d' % d)
def test_conv_image_unsupported_sizes_are_refused(dims):
    """A non-positive dimension, an even window and a window over 8 answer -3 from all three entry points."""
    from nnr_amd import _lib
    n, L, E, k = dims
    lib = _lib.lib()
    buf = torch.zeros(4096, device=dev())
    ids = torch.zeros(64, device=dev(), dtype=torch.int32)
    q = buf.data_ptr()
    assert lib.nnr_conv1d_image_fwd(q, 3, ids.data_ptr(), n, L, E, k, 0.0, 0, q, None) == _lib.NNR_ERR_UNSUPPORTED == -3
    assert lib.nnr_conv1d_dz_pad(q, q, n, L, E, k, q, None) == -3
    assert lib.nnr_conv1d_image_bwd(q, n, L, E, k, 0.0, 0, q, None) == -3


# ------------------------------------------------------------------------------------------------ the model
_SCALES = {}


def _full_size_scales(tag):
    """{parameter: max |gradient|} of a full-size fixture, from tests/naml_ref.py in float64 (computed once for both matrix paths)."""
    if tag not in _SCALES:
        from nnr_amd.model import Model
        from nnr_amd.synth import BATCH_FIELDS
        case = GoldenCase(tag)
        state = case.initial_state({k: tuple(p.shape) for k, p in Model(case.config, case.word_table()).named_parameters()})
        out = naml_ref.model_forward(case.config, state, {k: case.expect('in/' + k) for k in BATCH_FIELDS})
        out['loss'].backward()
        _SCALES[tag] = {k: float(p.grad.abs().max()) for k, p in out['state'].items()}
    return _SCALES[tag]


def _check_against_fixture(case, model, logits, loss):
    """logits, loss and every parameter gradient within 1e-4 of each tensor's scale (its max |expected|), every element.  Tiny fixtures:
    against the reference's float64 run.  The full-size fixture stores the fp32 run's 64-element slices, not the tensors: every stored
    element is compared, and the tensor's scale is read from the float64 restatement on the same weights and batch."""
    tiny = case.full_arrays
    pre = 'f64/' if tiny else ''
    report = []
    for name, got in (('logits', logits), ('loss', loss)):
        exp = np.asarray(case.expect(pre + name), dtype=np.float64)
        err, s = float(np.abs(got.detach().cpu().double().numpy() - exp).max()), float(np.abs(exp).max())
        report.append('%s %.2e / %.2e' % (name, err, s))
        assert err <= BAR * s, (name, err, s)
    for k, p in model.named_parameters():
        if k.startswith('user_encoder.news_encoder.'):
            continue
        ks = ZERO_ON_PAPER.get(k, k)
        s = float(np.abs(case.expect('f64/grad/' + ks)).max()) if tiny else _full_size_scales(case.tag)[ks]
        if tiny:
            exp, act = np.asarray(case.expect('f64/grad/' + k)), p.grad.detach().cpu().double().numpy()
        else:
            exp, act = case.expect_grad(k, p.grad)
        err = float(np.abs(act.reshape(exp.shape).astype(np.float64) - exp).max())
        report.append('%s %.2e / %.2e' % (k.replace('news_encoder.', 'ne.').replace('user_encoder.', 'ue.'), err, s))
        assert err <= BAR * s, (k, err, s)
    print('%s: %s' % (case.tag, '; '.join(report)))


@pytest.mark.parametrize('bx3', [True, False], ids=['bx3', 'f32_mfma'])
@pytest.mark.parametrize('tag', TINY + [FULL])
def test_model_matches_reference_golden(tag, bx3):
    """Step 0 of every fixture on both matrix paths (ops.BX3, the switch NNR_BX3 sets): logits, loss, every gradient element; then the
    fixture's Adam steps through the trainer: the loss of every step, and every parameter after the last step at the same bar of the
    parameter's scale (elements without a gradient on paper: see NOISE_FLOOR)."""
    from nnr_amd import ops
    from nnr_amd.model import negative_log_softmax
    from nnr_amd.trainer import Trainer
    case = GoldenCase(tag)
    steps = int(case.meta['adam_steps'])
    before = ops.BX3[0]
    ops.BX3[0] = bx3
    try:
        model, cfg = build_model(case, 'train')
        trainer = Trainer(model, cfg)
        for s in range(steps):
            batch = case.batch('cuda')
            trainer.flat.zero_grad()
            logits = model(*batch)
            loss = negative_log_softmax(logits)
            loss.backward()
            ops.join_extra_streams()
            torch.cuda.synchronize()
            if s == 0:
                for i, name in ((16, 'news_title_mask'), (19, 'news_content_mask'), (4, 'user_title_mask'), (7, 'user_content_mask')):
                    np.testing.assert_array_equal(batch[i].cpu().numpy(), case.expect('in/' + name))          # no mask is touched
                _check_against_fixture(case, model, logits, loss)
            assert abs(float(loss) - float(case.expect('loss_step%d' % s))) <= 5e-5, 'loss at step %d' % s
            trainer.optimizer_step(1.0)
        torch.cuda.synchronize()
    finally:
        ops.BX3[0] = before
    report, worst = [], {}
    for k, p in model.named_parameters():
        if k.startswith('user_encoder.news_encoder.'):
            continue
        exp, act = case.expect_param(steps, k, p)
        dlt = np.abs(act.reshape(exp.shape).astype(np.float64) - exp)
        noise = np.zeros(exp.shape, dtype=bool)
        if case.full_arrays:
            g64 = np.abs(case.expect('f64/grad/' + k))
            noise = g64 <= NOISE_FLOOR * float(np.abs(case.expect('f64/grad/' + ZERO_ON_PAPER.get(k, k))).max())
        s = float(np.abs(exp).max())
        worst[k] = (float(dlt[~noise].max(initial=0.0)), float(dlt[noise].max(initial=0.0)), s, int(noise.sum()))
        report.append('%s %.2e / %.2e' % (k.replace('news_encoder.', 'ne.').replace('user_encoder.', 'ue.'), worst[k][0], s) +
                      (' (+ %d zero-gradient elements: %.2e)' % (worst[k][3], worst[k][1]) if worst[k][3] else ''))
    print('%s after %d Adam steps: %s' % (tag, steps, '; '.join(report)))
    for k, (err, err_noise, s, _) in worst.items():
        assert err <= BAR * s, (k, err, s)
        assert err_noise <= steps * float(cfg.lr) * 1.01, (k, err_noise)


def test_dropout_on_matches_the_restatement_fed_the_kernels_masks():
    """NAML_Content + ATT in train mode at dropout 0.25: logits, loss and every gradient against the float64 restatement given the kernels'
    own keep-masks -- per encoder call the word rows at seed + 1 over the compact [n, L, E] and the convolution output at seed + 2 over the
    compact [n, L, C] (the masks nnr_embed_gather / nnr_dropout draw for those seeds)."""
    from hip_masks import _news_seed
    from nnr_amd import ops
    from nnr_amd.model import negative_log_softmax
    from nnr_amd.synth import BATCH_FIELDS
    case = GoldenCase('drop_tiny_NAML_Content_ATT')
    p = 0.25
    model, cfg = build_model(case, 'train')
    ne = model.news_encoder
    assert ne.training and ne.dropout_rate == p
    batch = case.batch('cuda')
    B, N, L = batch[18].shape
    H = batch[6].shape[1]
    E, C = int(cfg.word_embedding_dim), int(cfg.cnn_kernel_num)
    keeps = (naml_ref.site_masks(B * N, L, E, C, p, _news_seed(ne, 1)), naml_ref.site_masks(B * H, L, E, C, p, _news_seed(ne, 2)))
    for kd in keeps:
        for k, v in kd.items():
            assert 0.6 < float(v.float().mean()) < 0.9, k                                     # every site drops something
    logits = model(*batch)
    loss = negative_log_softmax(logits)
    loss.backward()
    ops.join_extra_streams()
    torch.cuda.synchronize()
    state = {k: v.detach().cpu().numpy() for k, v in model.named_parameters() if not k.startswith('user_encoder.news_encoder.')}
    out = naml_ref.model_forward(cfg, state, {k: case.expect('in/' + k) for k in BATCH_FIELDS}, p=p, keeps=keeps)
    out['loss'].backward()
    report = []
    for name, got, exp in (('logits', logits, out['logits']), ('loss', loss, out['loss'])):
        err, s = float((got.detach().cpu().double() - exp.detach()).abs().max()), float(exp.detach().abs().max())
        report.append('%s %.2e / %.2e' % (name, err, s))
        assert err <= BAR * s, (name, err, s)
    named = dict(model.named_parameters())
    for k, v in out['state'].items():
        err, s = float((named[k].grad.cpu().double() - v.grad).abs().max()), float(v.grad.abs().max())
        report.append('%s %.2e / %.2e' % (k, err, s))
        assert err <= BAR * s, (k, err, s)
    print('; '.join(report))


def test_compute_scores_and_metrics_match_reference():
    """evaluate.py with its news cache on (the encoders are batch-independent) and off: scores to the bars of the other encoders' eval
    tests, ranks equal."""
    from nnr_amd import evaluate as E
    z, model = eval_fixture('tiny_NAML_Title_ATT')
    model = model.cuda().train()
    assert E.news_reps_cacheable(model)
    dc = E.dev_corpus({k: z[k] for k in z.files}, 'cuda', int(z['category_num']))
    scores = E.compute_scores(model, dc, batch_size=int(z['batch_size']))
    assert model.training and E.LAST_STATS['mode'] == 'cached'
    got = scores.cpu().numpy()
    err = float(np.abs(got - z['scores']).max())
    smax = float(np.abs(z['scores']).max())
    print('eval_tiny_NAML_Title_ATT scores max-abs-err %.3e (max |score| %.3e)' % (err, smax))
    assert err <= LOGIT_TOL and err <= TIGHT * max(1.0, smax), err
    ranks, per, mean = E.rank_metrics(scores, torch.from_numpy(z['labels']), z['sizes'])
    np.testing.assert_array_equal(ranks.cpu().numpy(), z['ranks'])
    np.testing.assert_allclose(mean.cpu().numpy(), z['metrics'], rtol=0, atol=1e-12)
    uncached = E.compute_scores(model, dc, batch_size=int(z['batch_size']), cache=False)
    derr = float((uncached - scores).abs().max())
    assert derr <= LOGIT_TOL and derr <= TIGHT * max(1.0, smax), derr
    ranks2, _, _ = E.rank_metrics(uncached, torch.from_numpy(z['labels']), z['sizes'])
    np.testing.assert_array_equal(ranks2.cpu().numpy(), z['ranks'])


def test_backward_twice_gives_identical_bits():
    """The view attention's own gradients (both category tables, both affines, affine1 / affine2) of one history call at the full-size
    fixture's shapes: two passes from zeroed gradients, same bits; the representation too."""
    from nnr_amd import ops
    case = GoldenCase(FULL)
    model, cfg = build_model(case, 'train')
    enc = model.news_encoder
    b = case.batch('cuda')
    G = torch.randn(b[3].shape[0], b[3].shape[1], model.news_embedding_dim, generator=torch.Generator().manual_seed(1)).cuda()
    names = ['category_embedding.weight', 'subCategory_embedding.weight', 'category_affine.weight', 'category_affine.bias', 'subCategory_affine.weight',
             'subCategory_affine.bias', 'affine1.weight', 'affine1.bias', 'affine2.weight']
    runs = []
    for _ in range(2):
        for p in enc.parameters():
            p.grad = None
        rep = enc(b[3], b[4], b[5], b[6], b[7], b[8], b[1], b[2], None)
        (rep * G).sum().backward()
        ops.join_extra_streams()
        torch.cuda.synchronize()
        runs.append((rep.detach().clone(), {k: p.grad.clone() for k, p in enc.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in names:
        assert float(runs[0][1][k].abs().max()) > 0 and torch.equal(runs[0][1][k], runs[1][1][k]), k
