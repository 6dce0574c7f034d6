"""GPU tests of the KCNN news encoder (DKN): the kernels of csrc/kcnn.hip op by op against float64 / exact fp32 expectations, the encoder at
odd sizes against tests/kcnn_ref.py, and the model against the reference's own results (tests/golden/*KCNN*.npz) on both matrix paths."""
import functools

import numpy as np
import pytest
import torch

from golden_io import GoldenCase, build_model, eval_fixture
import kcnn_ref
from kcnn_ref import f64

pytestmark = pytest.mark.gpu

BAR = 1e-4                 # the project's headline bar: of each tensor's own scale (max |expected|), every element
LOGIT_TOL = 1e-4
TIGHT = 2e-5
TINY = ['tiny_KCNN_CATT', 'tiny_KCNN_ATT']
FULL = 'full_KCNN_CATT_g1p0'
IMAGE_SHAPES = [(3, 5, 8, 3), (2, 32, 300, 3), (1, 7, 6, 1), (2, 6, 10, 4), (2, 9, 12, 5)]          # (n, L, E, w)
# CATT's score bias shifts every history slot's score alike: the softmax does not see it and its gradient is zero on paper (3.5e-16 in the
# reference's float64 run).  What fp32 leaves there is the rounding of the terms that cancel, which are the terms of affine2.weight's
# gradient: that tensor's scale stands in.
ZERO_ON_PAPER = {'user_encoder.affine2.bias': 'user_encoder.affine2.weight'}


def dev():
    return torch.device('cuda')


def _ids(shape):
    return 'x'.join(str(v) for v in shape)


# ------------------------------------------------------------------------------------------------ image
def _image_inputs(n, L, E, w, seed):
    g = torch.Generator().manual_seed(seed)
    V = 23
    table = torch.randn(V, E, generator=g)
    text = torch.randint(0, V, (n, L), generator=g, dtype=torch.int32)
    text[0, -1] = 0
    pre1, pre2 = 1.5 * torch.randn(n * L, E, generator=g), 1.5 * torch.randn(n * L, E, generator=g)
    return table, text, pre1, pre2


@pytest.mark.parametrize('shape', IMAGE_SHAPES, ids=_ids)
def test_image_forward_and_backward(shape):
    """Forward: zero halo rows, channel 0 bit-equal to the table rows, the tanh channels within 1e-6 of float64, every element written
    (NaN prefill).  Backward: dx0 bit-equal to channel 0 of dXp; d pre = dXp * (1 - x^2) with x the fp32 image -- three fp32 roundings
    (x * x, 1 - ., the product), each at most 2^-24 of a result no larger than |dXp|: 4 * 2^-24 * max |dXp|; NaN in the halo rows of dXp
    (and of Xp) never reaches an output."""
    from nnr_amd import ops
    n, L, E, w = shape
    p, Lp = (w - 1) // 2, L + w - 1
    table, text, pre1, pre2 = _image_inputs(n, L, E, w, 7 + E)
    d = dev()
    Xp = torch.full((n * Lp, 3 * E), float('nan'), device=d)
    ops.kcnn_image_fwd(table.to(d), text.reshape(-1).to(d), pre1.to(d), pre2.to(d), n, L, w, Xp)
    X = Xp.cpu().view(n, Lp, 3, E)
    assert bool((X[:, :p] == 0).all()) and bool((X[:, p + L:] == 0).all()) and X[:, p + L:].shape[1] == w - 1 - p
    body = X[:, p:p + L]
    assert torch.equal(body[:, :, 0], table[text.long()])
    for j, pre in ((1, pre1), (2, pre2)):
        err = float((body[:, :, j].double() - torch.tanh(pre.double()).view(n, L, E)).abs().max())
        print('image %s channel %d: max |err| %.2e' % (_ids(shape), j, err))
        assert err <= 1e-6
    g = torch.Generator().manual_seed(3)
    dX = 0.25 * torch.randn(n, Lp, 3, E, generator=g)
    halo = torch.ones(Lp, dtype=torch.bool)
    halo[p:p + L] = False
    dX[:, halo] = float('nan')
    Xn = X.clone()
    Xn[:, halo] = float('nan')
    outs = [torch.full((n * L, E), float('nan'), device=d) for _ in range(3)]
    ops.kcnn_image_bwd(dX.reshape(n * Lp, 3 * E).to(d), Xn.reshape(n * Lp, 3 * E).to(d), n, L, E, w, *outs)
    dx0, dp1, dp2 = (o.cpu().view(n, L, E) for o in outs)
    gb = dX[:, p:p + L]
    assert torch.equal(dx0, gb[:, :, 0])
    bar = 4 * 2.0 ** -24 * float(gb.abs().max())
    for j, got in ((1, dp1), (2, dp2)):
        exp = gb[:, :, j].double() * (1.0 - body[:, :, j].double() ** 2)
        err = float((got.double() - exp).abs().max())
        print('image bwd %s channel %d: max |err| %.2e (bar %.2e)' % (_ids(shape), j, err, bar))
        assert bool(torch.isfinite(got).all()) and err <= bar


# ------------------------------------------------------------------------------------------------ window max
def _window_case(n, C, L, w, seed, ldz):
    """z [n * Lp, ldz] on a grid of eighths with distinct, well separated entries per (title, channel), bias in eighths: fl(z + b) is exact.
    Title 0: all-negative columns; title 1: the maximum at t = 0; title 2: at t = L - w; the rows the pool never sees hold +100."""
    g = torch.Generator().manual_seed(seed)
    Lp, T = L + w - 1, L - w + 1
    order = torch.argsort(torch.rand(n, C, Lp, generator=g), dim=2).permute(0, 2, 1).float()          # a permutation of 0..Lp-1 per (title, channel)
    z = 0.5 * order - 0.25 * Lp + 0.125 * torch.randint(0, 3, (n, 1, C), generator=g).float()
    z[0] = -1.0 - 0.5 * order[0]
    if n > 2:
        z[1, 0], z[2, T - 1] = 50.0, 60.0
    z[:, T:] = 100.0
    bias = 0.125 * torch.randint(-8, 9, (C,), generator=g).float()
    full = torch.full((n * Lp, ldz), float('nan'))
    full[:, :C] = z.reshape(n * Lp, C)
    return z, bias, full


@pytest.mark.parametrize('shape', [(19, 400, 7, 3, 400), (5, 6, 32, 3, 9), (9, 130, 6, 4, 130), (3, 6, 5, 1, 6), (8, 130, 9, 5, 132),
                                   (30, 6, 7, 3, 6), (33, 70, 5, 3, 70)], ids=_ids)
def test_window_max_forward_and_backward_are_exact(shape):
    """out, arg, dz and db equal torch's fp32 relu-then-max over the first L - w + 1 positions EXACTLY (grid values: every sum is exact, every
    maximum unique); arg = 255 and a zero gradient where nothing is positive; dz and db are prefilled with NaN: every element is written,
    the leading rows included.  db sums one partial row per 8 titles: the title counts cover 1, 2, 3, 4 and 5 rows."""
    from nnr_amd import ops
    n, C, L, w, ldz = shape
    Lp, T = L + w - 1, L - w + 1
    z, bias, full = _window_case(n, C, L, w, 11 + C, ldz)
    d = dev()
    out = torch.full((n, C), float('nan'), device=d)
    arg = torch.full((n, C), 77, device=d, dtype=torch.uint8)
    ops.window_max_fwd(full.to(d), ldz, bias.to(d), n, C, L, w, out, arg)
    r = torch.relu(z + bias)[:, :T]
    top, idx = r.max(dim=1)
    exp_arg = torch.where(top > 0, idx, torch.full_like(idx, 255)).to(torch.uint8)
    assert torch.equal(out.cpu(), top) and torch.equal(arg.cpu(), exp_arg)
    assert bool((exp_arg[0] == 255).all()) and (n <= 2 or (bool((exp_arg[1] == 0).all()) and bool((exp_arg[2] == T - 1).all())))
    g = 0.125 * torch.randint(-40, 41, (n, C), generator=torch.Generator().manual_seed(5)).float()
    for lead in (0, w - 1):
        dz = torch.full((lead + n * Lp, C), float('nan'), device=d)
        db = torch.full((C,), float('nan'), device=d)
        ops.window_max_bwd(g.to(d), arg, n, C, L, w, lead, dz, db)
        exp = torch.zeros(n, Lp, C)
        live = exp_arg != 255
        ii, cc = torch.nonzero(live, as_tuple=True)
        exp[ii, exp_arg[ii, cc].long(), cc] = g[ii, cc]
        got = dz.cpu()
        assert bool((got[:lead] == 0).all()) and torch.equal(got[lead:], exp.reshape(n * Lp, C))
        assert torch.equal(db.cpu(), (g * live).sum(dim=0))


def test_repack_round_trip_is_exact():
    """ops.permute (nnr_permute) over the seven layouts of ops.LAYOUTS at the host test's sizes, plus the default KCNN weight (1.08 M elements:
    past one pass of the 4096-block grid): the destination, prefilled with NaN, equals the CPU permutation bit for bit -- its pad columns
    still NaN --, the source is unchanged, and a gradient kind added twice into a zeroed buffer gives W, then 2 W (its source is W's
    permuted form with NaN in the pad columns: they are never read)."""
    from nnr_amd import ops
    import layout_ref
    d = dev()
    for kind, dims in layout_ref.CASES + [(k, (400, 300, 3)) for k in ('kcnn_p', 'kcnn_q', 'kcnn_dw')]:
        shape = ops.LAYOUTS[kind](*dims)[4]
        nan = torch.full(shape, float('nan'))
        if kind.endswith('_dw'):
            fwd = kind[:-2] + 'p'
            W = layout_ref.source(fwd, dims)
            src = layout_ref.expected(fwd, W, dims, torch.full(ops.LAYOUTS[fwd](*dims)[4], float('nan')))
            sd, out = src.to(d), torch.zeros(shape, device=d)
            for times in (1, 2):
                ops.permute(sd, out, kind, dims, accumulate=True)
                assert torch.equal(out.cpu(), times * W), (kind, dims, times)
        else:
            src = layout_ref.source(kind, dims)
            sd, out = src.to(d), nan.to(d)
            ops.permute(sd, out, kind, dims)
            exp, got = layout_ref.expected(kind, src, dims, nan), out.cpu()
            pad = torch.isnan(exp)
            assert torch.equal(torch.isnan(got), pad) and torch.equal(got[~pad], exp[~pad]), (kind, dims)
            assert bool(pad.any()) == (exp.numel() != src.numel())          # rows of ldp > C floats, of Cout / Cin rounded up to 4
        assert torch.equal(sd.cpu().nan_to_num(nan=7.0), src.nan_to_num(nan=7.0))
    # served through the derived-weight cache, the Conv3d operands' pad columns are zero: after the first serve and after the weight changed
    for Cout, Cin, K in layout_ref.C3_DIMS:
        w = torch.nn.Parameter(layout_ref.source('c3_p', (Cout, Cin, K)).view(Cout, Cin, K, K, K).to(d))
        for step in range(2):
            for mode, kind in enumerate(('c3_p', 'c3_q')):
                got = ops.conv3d_weight(w, mode)
                exp = layout_ref.expected(kind, w.detach().cpu().view(Cout, Cin, K ** 3), (Cout, Cin, K), torch.zeros(got.shape))
                assert torch.equal(got.cpu(), exp), (kind, Cout, Cin, K, step)
            with torch.no_grad():
                w.mul_(-1.5)


@pytest.mark.parametrize('dims', [(254, 8, 3), (16, 8, 9), (5, 1028, 3), (3, 8, 4)], ids=_ids)
def test_sizes_beyond_the_limits_are_unsupported(dims):
    """L + w - 1 > 255, w > 8, E > 1024 and L < w raise instead of launching."""
    from nnr_amd import ops, _lib
    L, E, w = dims
    d = dev()
    n, C, Lp = 1, 4, L + w - 1
    table, text = torch.zeros(3, E, device=d), torch.zeros(n * L, device=d, dtype=torch.int32)
    pre = torch.zeros(n * L, E, device=d)
    Xp = torch.zeros(n * Lp, 3 * E, device=d)
    with pytest.raises(_lib.NnrHipError, match='unsupported size'):
        ops.kcnn_image_fwd(table, text, pre, pre, n, L, w, Xp)
    with pytest.raises(_lib.NnrHipError, match='unsupported size'):
        ops.kcnn_image_bwd(Xp, Xp, n, L, E, w, pre.clone(), pre.clone(), pre.clone())
    if E <= 1024:
        z = torch.zeros(n * Lp, C, device=d)
        with pytest.raises(_lib.NnrHipError, match='unsupported size'):
            ops.window_max_fwd(z, C, torch.zeros(C, device=d), n, C, L, w, torch.zeros(n, C, device=d), torch.zeros(n, C, device=d, dtype=torch.uint8))
        with pytest.raises(_lib.NnrHipError, match='unsupported size'):
            ops.window_max_bwd(torch.zeros(n, C, device=d), torch.zeros(n, C, device=d, dtype=torch.uint8), n, C, L, w, 0, z, torch.zeros(C, device=d))
    if w > 8 or E > 1024:
        with pytest.raises(_lib.NnrHipError, match='unsupported size'):
            ops.rowconv_weight(torch.zeros(C, E, w, 3, device=d), 0)


# ------------------------------------------------------------------------------------------------ the encoder at odd sizes
ENCODER_CASES = [dict(L=6, E=10, w=4, C=6, De=5, Dc=7, B=2, N=3, seed=1), dict(L=9, E=12, w=5, C=130, De=8, Dc=4, B=3, N=2, seed=21),
                 dict(L=7, E=16, w=1, C=12, De=6, Dc=6, B=2, N=2, seed=3)]      # (seeds: the first whose float64 margins reach 1e-3 of the scale)


@pytest.mark.parametrize('c', ENCODER_CASES, ids=lambda c: 'L%d_E%d_w%d_C%d' % (c['L'], c['E'], c['w'], c['C']))
def test_encoder_matches_the_float64_restatement_at_odd_sizes(c):
    """One KCNN call (even and unit windows, E no multiple of 4, C over one block) against tests/kcnn_ref.py: the representation and every
    parameter gradient of (rep * G).sum() within 1e-4 of each tensor's scale, every element.  The float64 margins of the case are asserted
    first (1e-3 of the scale, as the fixtures'), so no argmax flip is excused."""
    from nnr_amd.config import make_config
    from nnr_amd import news_encoders as NE
    V, S = 31, 9
    cfg = make_config(['--news_encoder=KCNN', '--user_encoder=ATT', '--max_title_length=%d' % c['L'], '--word_embedding_dim=%d' % c['E'],
                       '--cnn_window_size=%d' % c['w'], '--cnn_kernel_num=%d' % c['C'], '--entity_embedding_dim=%d' % c['De'],
                       '--context_embedding_dim=%d' % c['Dc'], '--category_embedding_dim=4', '--subCategory_embedding_dim=4'],
                      corpus_sizes=dict(vocabulary_size=V, entity_size=S, category_num=3, subCategory_num=5), dropout_rate=0.0)
    torch.manual_seed(c['seed'])
    enc = NE.KCNN(cfg, 0.5 * torch.randn(V, c['E']), 0.5 * torch.randn(S, c['De']), 0.5 * torch.randn(S, c['Dc']))
    enc.initialize()
    with torch.no_grad():
        enc.knowledge_cnn.conv.weight.mul_(3.0)
        enc.knowledge_cnn.conv.bias.normal_(0.0, 0.2)
    B, N, L = c['B'], c['N'], c['L']
    g = torch.Generator().manual_seed(c['seed'] + 10)
    text = torch.randint(0, V, (B, N, L), generator=g, dtype=torch.int32)
    ent = torch.randint(0, S, (B, N, L), generator=g, dtype=torch.int32) * (torch.rand(B, N, L, generator=g) < 0.3).int()
    cat, sub = torch.randint(0, 3, (B, N), generator=g, dtype=torch.int32), torch.randint(0, 5, (B, N), generator=g, dtype=torch.int32)
    G = torch.randn(B, N, c['C'] + 8, generator=g)
    st = {'news_encoder.' + k: f64(p).requires_grad_() for k, p in enc.named_parameters()}
    rep64, z = kcnn_ref.kcnn_call(st, text, ent, cat, sub)
    (rep64 * G.double()).sum().backward()
    top, gap, _ = kcnn_ref.margins(z, c['w'], text.reshape(B * N, L), ent.reshape(B * N, L))
    scale = float(torch.relu(z.detach()).max())
    assert float(gap[top > 0].min()) >= 1e-3 * scale, (float(gap[top > 0].min()), scale)
    enc = enc.cuda().train()
    d = dev()
    mask = torch.ones(B, N, L, dtype=torch.bool, device=d)
    rep = enc(text.to(d), mask, ent.to(d), None, None, None, cat.to(d), sub.to(d), None)
    (rep * G.to(d)).sum().backward()
    from nnr_amd import ops
    ops.join_extra_streams()
    torch.cuda.synchronize()
    err, s = float((rep.detach().cpu().double() - rep64.detach()).abs().max()), float(rep64.detach().abs().max())
    print('rep err %.2e of scale %.2e' % (err, s))
    assert err <= BAR * s
    for k, p in enc.named_parameters():
        exp = st['news_encoder.' + k].grad
        err, s = float((p.grad.cpu().double() - exp).abs().max()), float(exp.abs().max())
        print('grad %s err %.2e of scale %.2e' % (k, err, s))
        assert err <= BAR * s, k


# ------------------------------------------------------------------------------------------------ the model
@functools.lru_cache(maxsize=None)
def _full_size_scales(tag):
    """{parameter: max |gradient|} of a full-size fixture, from tests/kcnn_ref.py in float64 (computed once for both matrix paths)."""
    from nnr_amd.model import Model
    from nnr_amd.synth import BATCH_FIELDS
    case = GoldenCase(tag)
    state = case.initial_state({k: tuple(p.shape) for k, p in Model(case.config, case.word_table()).named_parameters()})
    out = kcnn_ref.model_forward(case.config, state, {k: case.expect('in/' + k) for k in BATCH_FIELDS})
    out['loss'].backward()
    return {k: float(p.grad.abs().max()) for k, p in out['state'].items()}


def _check_against_fixture(case, model, logits, loss):
    """logits, loss and every parameter gradient within 1e-4 of each tensor's scale (its max |expected|), every element.  Tiny fixtures: against
    the reference's float64 run.  The full-size fixture stores the fp32 run's 64-element slices, not the tensors: every stored element is
    compared, and the tensor's scale is read from the float64 restatement on the same weights and batch (_full_size_scales)."""
    tiny = case.full_arrays
    pre = 'f64/' if tiny else ''
    report = []
    for name, got in (('logits', logits), ('loss', loss)):
        exp = np.asarray(case.expect(pre + name), dtype=np.float64)
        err, s = float(np.abs(got.detach().cpu().double().numpy() - exp).max()), float(np.abs(exp).max())
        report.append('%s %.2e / %.2e' % (name, err, s))
        assert err <= BAR * s, (name, err, s)
    scales = {}
    for k, p in model.named_parameters():
        if k.startswith('user_encoder.news_encoder.'):
            continue
        scales[k] = float(np.abs(case.expect('f64/grad/' + k)).max()) if tiny else _full_size_scales(case.tag)[k]
    for k, p in model.named_parameters():
        if k not in scales:
            continue
        if tiny:
            exp, act = np.asarray(case.expect('f64/grad/' + k)), p.grad.detach().cpu().double().numpy()
        else:
            exp, act = case.expect_grad(k, p.grad)
        s = scales[ZERO_ON_PAPER.get(k, k)]
        err = float(np.abs(act.reshape(exp.shape).astype(np.float64) - exp).max())
        report.append('%s %.2e / %.2e' % (k.replace('news_encoder.', 'ne.').replace('user_encoder.', 'ue.'), err, s))
        assert err <= BAR * s, (k, err, s)
    print('%s: %s' % (case.tag, '; '.join(report)))


@pytest.mark.parametrize('bx3', [True, False], ids=['bx3', 'f32_mfma'])
@pytest.mark.parametrize('tag', TINY + [FULL])
def test_model_matches_reference_golden(tag, bx3):
    """Both matrix paths (ops.BX3, the switch NNR_BX3 sets: the convolution products of the full-size fixture are long enough for the bf16x3
    kernel), the step's side-stream branch included at full size."""
    from nnr_amd import ops
    from nnr_amd.model import negative_log_softmax
    case = GoldenCase(tag)
    before = ops.BX3[0]
    ops.BX3[0] = bx3
    try:
        model, cfg = build_model(case, 'train')
        assert model.news_encoder.auxiliary_loss is None
        batch = case.batch('cuda')
        logits = model(*batch)
        loss = negative_log_softmax(logits)
        loss.backward()
        ops.join_extra_streams()
        torch.cuda.synchronize()
    finally:
        ops.BX3[0] = before
    np.testing.assert_array_equal(batch[16].cpu().numpy(), case.expect('in/news_title_mask'))          # no mask is touched
    _check_against_fixture(case, model, logits, loss)


def test_model_on_the_side_stream_branch_equals_the_sequential_one():
    """Model.forward issues the candidate call on a side stream when the step counts as GPU-bound (forced by the threshold): both calls'
    plain (non-atomic) gradient writers -- the bias add, the weight unpack -- then come from two streams and must not overlap."""
    from nnr_amd import ops
    from nnr_amd.model import negative_log_softmax
    case = GoldenCase(TINY[0])
    old = ops.LEAF_MIN_ROWS
    ops.LEAF_MIN_ROWS = 1
    try:
        model, cfg = build_model(case, 'train')
        logits = model(*case.batch('cuda'))
        loss = negative_log_softmax(logits)
        loss.backward()
        ops.join_extra_streams()
        torch.cuda.synchronize()
    finally:
        ops.LEAF_MIN_ROWS = old
    _check_against_fixture(case, model, logits, loss)


def test_backward_twice_gives_identical_bits():
    """The encoder's own gradients (three tables, both projections, the convolution) of one call at the full-size fixture's shapes, long
    enough for split-K: two passes from zeroed gradients, same bits."""
    from nnr_amd import ops
    case = GoldenCase(FULL)
    model, cfg = build_model(case, 'train')
    enc = model.news_encoder
    b = case.batch('cuda')
    G = torch.randn(b[3].shape[0], b[3].shape[1], model.news_embedding_dim, generator=torch.Generator().manual_seed(1)).cuda()
    names = [k for k, _ in enc.named_parameters() if 'category' not in k.lower()]
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


def test_trainer_steps_move_the_tables_and_the_convolution():
    """Trainer.train_step twice with CATT (autograd path, no tape): the losses are the reference's, and all three tables, both projections
    and the convolution move."""
    from nnr_amd.trainer import Trainer
    case = GoldenCase(TINY[0])
    model, cfg = build_model(case, 'train')
    trainer = Trainer(model, cfg)
    watched = ['news_encoder.%s.weight' % k for k in ('word_embedding', 'entity_embedding', 'context_embedding', 'M_entity', 'M_context', 'knowledge_cnn.conv')]
    before = {k: p.detach().clone() for k, p in model.named_parameters() if k in watched}
    assert len(before) == len(watched)
    for s in range(2):
        _, loss = trainer.train_step(case.batch('cuda'))
        assert trainer.last_path == 'autograd'
        assert abs(float(loss) - float(case.expect('loss_step%d' % s))) <= 5e-5, 'loss at step %d' % s
    torch.cuda.synchronize()
    assert not trainer.tapes and bool(torch.isfinite(loss))
    after = dict(model.named_parameters())
    for k in watched:
        moved = float((after[k].detach() - before[k]).abs().max())
        assert moved > 1e-3, (k, moved)                        # (two Adam steps at lr 1e-2 move a parameter with gradient by about 2e-2)


def test_compute_scores_and_metrics_match_reference():
    """evaluate.py with its news cache on (KCNN is batch-independent), to the bars of the other encoders' eval tests."""
    from nnr_amd import evaluate as E
    z, model = eval_fixture('tiny_KCNN_CATT')
    model = model.cuda().train()
    assert E.news_reps_cacheable(model)
    dc = E.dev_corpus({k: z[k] for k in z.files}, 'cuda', int(z['category_num']))
    scores = E.compute_scores(model, dc, batch_size=int(z['batch_size']))
    assert model.training and E.LAST_STATS['mode'] == 'cached'
    got = scores.cpu().numpy()
    err = float(np.abs(got - z['scores']).max())
    smax = float(np.abs(z['scores']).max())
    print('eval_tiny_KCNN_CATT scores max-abs-err %.3e (max |score| %.3e)' % (err, smax))
    assert err <= LOGIT_TOL and err <= TIGHT * max(1.0, smax), err
    ranks, per, mean = E.rank_metrics(scores, torch.from_numpy(z['labels']), z['sizes'])
    np.testing.assert_array_equal(ranks.cpu().numpy(), z['ranks'])
    np.testing.assert_allclose(mean.cpu().numpy(), z['metrics'], rtol=0, atol=1e-12)
    uncached = E.compute_scores(model, dc, batch_size=int(z['batch_size']), cache=False)
    derr = float((uncached - scores).abs().max())
    assert derr <= LOGIT_TOL and derr <= TIGHT * max(1.0, smax), derr
