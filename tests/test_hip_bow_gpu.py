"""The bag-of-words news encoders on the GPU: the bag kernels (csrc/bag.hip), the row distance, the sigmoid dense layer, and the DAE /
Inception models, plug-in, evaluation and dropout-on paths.

Bars.  Op tests: for each op and shape the same formula is evaluated in fp32 by CPU torch and compared with the float64 restatement of
tests/bow_ref.py (pinned to the reference by tests/test_bow_host.py); the kernel's bar is 4 x that error (the factor covers another
summation order), never below 1e-6 x the expected tensor's max magnitude.  Every measured value is printed (profiles/bow_summary.md keeps
them).  Model tests: the bars of tests/test_hip_npa_gpu.py's model test, unchanged."""

import numpy as np
import pytest
import torch

from golden_io import GoldenCase, build_model, eval_fixture
import bow_ref
from bow_ref import f64

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4
TIGHT = 2e-5
TINY = ['tiny_DAE_ATT', 'tiny_DAE_CATT', 'tiny_Inception_ATT', 'tiny_Inception_CATT']
CASES = TINY + ['full_DAE_ATT_g1p0', 'full_Inception_ATT_g1p0']
# (n, La, Lb, E, V): the smallest case | E % 4 != 0 with one stream | MIND widths, n no multiple of the 4 waves of a workgroup, two ballots,
# heavy duplication | three words: segments of thousands of occurrences that span several workgroups' partial rows | beyond the issue's four:
# odd E (the scalar-lane forward instantiation) | ONE word: a segment of ~4 300 occurrences = ~135 chunks, more than the 64 one window of the
# second backward pass walks (its multi-window path)
BAG_SHAPES = [(1, 5, 9, 16, 64), (7, 5, None, 50, 64), (67, 32, 128, 300, 64), (67, 32, 128, 300, 3), (6, 5, 9, 15, 64), (67, 32, 128, 300, 1)]
MODES = [('joint', 'sigmoid'), ('joint', 'none'), ('separate', 'none'), ('separate', 'sigmoid')]


def _bar(exp, fp32, name, report):
    """4 x the error of the same formula in fp32 on the CPU, floor 1e-6 x max |expected|."""
    e32, emax = float((fp32.double() - exp).abs().max()), float(exp.abs().max())
    bar = max(4.0 * e32, 1e-6 * emax)
    report.append('%s: fp32 formula %.3e, max|exp| %.3e, bar %.3e' % (name, e32, emax, bar))
    return bar


def _bag_inputs(n, La, Lb, E, V, separate, seed):
    """Masks are random bit patterns (holes, not prefixes).  Rows, as far as n reaches: row 0 at full length in both streams, with a live id 0
    and an id repeated inside the row; row 1 with an empty second stream; row 2 with only position 0 live; row 3 with an empty FIRST stream.
    n = 1 keeps row 0 only, so the one-row shape adds the other three patterns as extra rows of a second call (see the test).  In joint mode
    every row keeps a live position (a row without one is the reference's 0 / 0, not tested)."""
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(V, E, generator=g)
    ids = [torch.randint(0, V, (n, L), generator=g, dtype=torch.int32) for L in (La, Lb) if L]
    masks = [torch.rand(n, L, generator=g) < 0.4 for L in (La, Lb) if L]
    for m in masks:
        m[torch.arange(n), torch.randint(0, m.shape[1], (n,), generator=g)] = True
    for m, i in zip(masks, ids):
        m[0] = True
        i[0, 0] = 0
        if m.shape[1] > 2:
            i[0, 2] = i[0, 1]
    if n > 1 and Lb:
        masks[1][1] = False
    if n > 2:
        for m in masks:
            m[2] = False
            m[2, 0] = True
    if n > 3 and Lb:
        masks[0][3] = False
    dout = torch.randn(n, (2 if separate and Lb else 1) * E, generator=g)
    prefill = 0.1 * torch.randn(V, E, generator=g)
    return table, ids, masks, dout, prefill


def _bag_expected(table, ids, masks, dout, prefill, separate, sigmoid, dtype):
    t = table.detach().clone().to(dtype).requires_grad_()
    two = len(ids) == 2
    out = bow_ref.bag_mean(t, ids[0], masks[0], ids[1] if two else None, masks[1] if two else None, separate=separate, sigmoid=sigmoid)
    if separate:
        out = torch.cat([o for o in out if o is not None], dim=1)
    (out * dout.to(dtype)).sum().backward()
    return out.detach(), prefill.to(dtype) + t.grad


def _bag_run(table, ids, masks, dout, prefill, separate, sigmoid, runs=1):
    from nnr_amd import ops
    n, La = ids[0].shape
    two = len(ids) == 2
    Lb = ids[1].shape[1] if two else 0
    V, E = table.shape
    dev = dict(device='cuda', dtype=torch.float32)
    td = table.cuda()
    idd = [i.cuda().contiguous() for i in ids]
    md = [m.cuda().contiguous() for m in masks]
    act = ops.ACT_SIGMOID if sigmoid else ops.ACT_NONE
    # separate mode: two column slices of one wider buffer with an odd leading dimension, as Inception's [n, 4E] buffer is used
    ldo, off_a, off_b = (2 * E + 9, 3, E + 5) if separate else (E, 0, 0)
    out, count = torch.full((n, ldo), 7.0, **dev), torch.empty(2 * n if separate else n, **dev)
    plan = ops.BagPlan(n, La, Lb, V, torch.device('cuda'))
    rc = ops.bag_mean_fwd(td, idd[0], md[0], idd[1] if two else None, md[1] if two else None, separate, act, out, ldo, off_a, off_b, count, plan)
    assert rc == 0, rc
    plan.sort()
    douts = torch.zeros((n, ldo), **dev)
    douts[:, off_a:off_a + E] = dout[:, :E].cuda()
    if separate and two:
        douts[:, off_b:off_b + E] = dout[:, E:].cuda()
    tables = []
    for _ in range(runs):
        dt = prefill.cuda().clone()
        ops.bag_mean_bwd(douts, ldo, out, ldo, off_a, off_b, count, plan, separate, act, dt)
        tables.append(dt)
    torch.cuda.synchronize()
    got = torch.cat([out[:, off_a:off_a + E]] + ([out[:, off_b:off_b + E]] if separate and two else []), dim=1)
    return dict(out=got, dtable=tables, count=count, masks=md, tok=plan.tok.view(n, La + Lb), buf=out, cols=(ldo, off_a, off_b))


@pytest.mark.parametrize('shape', BAG_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
@pytest.mark.parametrize('mode', MODES, ids=lambda m: '-'.join(m))
def test_bag_kernels_match_the_float64_restatement(shape, mode):
    n, La, Lb, E, V = shape
    separate, sigmoid = mode[0] == 'separate', mode[1] == 'sigmoid'
    sets = [_bag_inputs(n, La, Lb, E, V, separate, seed=sum(v or 0 for v in shape) + 3 * separate + sigmoid)]
    if n == 1:                                       # the patterns of rows 1..3, which one row cannot hold
        sets.append(_bag_inputs(4, La, Lb, E, V, separate, seed=91 + 3 * separate + sigmoid))
    report = []
    for inp in sets:
        table, ids, masks, dout, prefill = inp
        exp_out, exp_dt = _bag_expected(*inp, separate, sigmoid, torch.float64)
        f32_out, f32_dt = _bag_expected(*inp, separate, sigmoid, torch.float32)
        got = _bag_run(*inp, separate, sigmoid, runs=2)
        bars = dict(out=_bar(exp_out, f32_out, 'out', report), dtable=_bar(exp_dt, f32_dt, 'dtable', report))
        errs = dict(out=float((got['out'].cpu().double() - exp_out).abs().max()), dtable=float((got['dtable'][0].cpu().double() - exp_dt).abs().max()))
        report.append('kernel: out %.3e, dtable %.3e' % (errs['out'], errs['dtable']))
        print('%s %s: %s' % (shape, mode, '; '.join(report)))
        assert errs['out'] <= bars['out'] and errs['dtable'] <= bars['dtable'], (shape, mode, errs, bars)
        assert torch.equal(got['dtable'][0], got['dtable'][1])                       # same inputs, same bits
        # the pre-filled table rows no live occurrence names keep their bits
        live = [(m.clone() if not separate else torch.cat([torch.ones(m.shape[0], 1, dtype=torch.bool), m[:, 1:]], dim=1)) for m in masks]
        used = torch.zeros(V, dtype=torch.bool)
        for i, m in zip(ids, live):
            used[i[m].long()] = True
        assert torch.equal(got['dtable'][0].cpu()[~used], prefill[~used])
        # counts, occurrence keys, masks, and the columns of the output buffer outside the two slices
        cnt = torch.cat([m.sum(dim=1).float() for m in live]) if separate else sum(m.sum(dim=1).float() for m in live)
        assert torch.equal(got['count'].cpu()[:cnt.numel()], cnt)
        tok = torch.cat([torch.where(m, i, torch.full_like(i, -1)) for i, m in zip(ids, live)], dim=1)
        assert torch.equal(got['tok'].cpu(), tok)
        for m_dev, m0, m1 in zip(got['masks'], masks, live):
            assert torch.equal(m_dev.cpu(), m1 if separate else m0)                 # joint: bytes unchanged; separate: mask[:, 0] = 1, the rest unchanged
            if separate:
                assert bool(m_dev[:, 0].all())
        ldo, off_a, off_b = got['cols']
        keep = torch.ones(ldo, dtype=torch.bool)
        keep[off_a:off_a + E] = False
        if separate and len(ids) == 2:
            keep[off_b:off_b + E] = False
        assert int(torch.count_nonzero(got['buf'].cpu()[:, keep] != 7.0)) == 0


def test_bag_sizes_beyond_the_limits_are_unsupported():
    """More than 128 positions in a stream (two ballots) or more than 320 columns (five per lane in the backward pass): NNR_ERR_UNSUPPORTED
    before any launch, which ops.bag_mean_fwd turns into an error (there is no fallback); the autograd function passes it on."""
    from nnr_amd import ops, _lib
    from nnr_amd import functional as Fn
    dev = dict(device='cuda')
    for La, Lb, E in ((129, 9, 16), (5, 129, 16), (5, 9, 324)):
        table = torch.zeros(8, E, **dev)
        ia, ib = torch.zeros(2, La, dtype=torch.int32, **dev), torch.zeros(2, Lb, dtype=torch.int32, **dev)
        ma, mb = torch.ones(2, La, dtype=torch.bool, **dev), torch.ones(2, Lb, dtype=torch.bool, **dev)
        out, count = torch.empty(2, E, **dev), torch.empty(2, **dev)
        with pytest.raises(_lib.NnrHipError, match='unsupported size'):
            ops.bag_mean_fwd(table, ia, ma, ib, mb, False, ops.ACT_NONE, out, E, 0, 0, count)
        with pytest.raises(_lib.NnrHipError, match='unsupported size'):
            Fn.BagMeanFn.apply(table, ia, ma, ib, mb, ops.ACT_NONE, False)


# ------------------------------------------------------------------------------------------------ row distance
@pytest.mark.parametrize('shape', [(1, 16), (5, 50), (67, 300)], ids=lambda s: 'x'.join(map(str, s)))
def test_row_dist_matches_torch_norm(shape):
    """Expected values from torch.norm in float64 (its subgradient at a == b is zero, tests/test_bow_host.py).  One row has a == b; the
    one-row shape runs both with and without it."""
    from nnr_amd import ops
    n, D = shape
    coef = 0.1
    for equal_row in ([True, False] if n == 1 else [True]):
        g = torch.Generator().manual_seed(n + D + equal_row)
        a, b, gup = torch.randn(n, D, generator=g), torch.randn(n, D, generator=g), torch.randn(n, generator=g)
        pa, pb = torch.randn(n, D, generator=g), torch.randn(n, D, generator=g)
        if equal_row:
            b[n // 2] = a[n // 2]

        def formula(dtype):
            x, y = a.clone().to(dtype).requires_grad_(), b.clone().to(dtype).requires_grad_()
            aux = torch.norm(x - y, dim=1) * coef
            (aux * gup.to(dtype)).sum().backward()
            return aux.detach(), pa.to(dtype) + x.grad, pb.to(dtype) + y.grad
        exp, f32 = formula(torch.float64), formula(torch.float32)
        ad, bd = a.cuda(), b.cuda()
        dist, aux = torch.empty(n, device='cuda'), torch.empty(n, device='cuda')
        ops.row_dist_fwd(ad, bd, coef, dist, aux)
        da, db = pa.cuda().clone(), pb.cuda().clone()
        ops.row_dist_bwd(ad, bd, dist, gup.cuda(), coef, da, db)
        torch.cuda.synchronize()
        report = []
        for name, got, e, f in zip(('aux', 'da', 'db'), (aux, da, db), exp, f32):
            bar = _bar(e, f, name, report)
            err = float((got.cpu().double() - e).abs().max())
            report.append('kernel %s %.3e' % (name, err))
            assert err <= bar, (shape, name, err, bar)
        print('%s equal_row=%s: %s' % (shape, equal_row, '; '.join(report)))
        assert bool(torch.isfinite(aux).all() and torch.isfinite(da).all() and torch.isfinite(db).all())
        if equal_row:
            r = n // 2
            assert float(aux[r]) == 0.0 and torch.equal(da[r].cpu(), pa[r]) and torch.equal(db[r].cpu(), pb[r])     # zero gradient: the pre-filled bits


# ------------------------------------------------------------------------------------------------ dense layer with a sigmoid
@pytest.mark.parametrize('shape', [(7, 50, 12), (67, 300, 200)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('p', [0.0, 0.2])
def test_linear_fn_with_sigmoid(shape, p):
    from nnr_amd import ops
    from nnr_amd import functional as Fn
    from hip_masks import flat_keep
    M, K, N = shape
    seed = 4242 + M
    torch.manual_seed(M + N)
    lin = torch.nn.Linear(K, N).cuda()
    x, dy = torch.randn(M, K), torch.randn(M, N)
    keep = flat_keep(M * N, p, seed).view(M, N).cpu()
    if p > 0:
        assert 0.6 < float(keep.float().mean()) < 0.95

    def formula(dtype):
        xx = x.clone().to(dtype).requires_grad_()
        w, b = lin.weight.detach().cpu().to(dtype).requires_grad_(), lin.bias.detach().cpu().to(dtype).requires_grad_()
        y = bow_ref.linear(xx, w, b, 'sigmoid', keep, p)
        (y * dy.to(dtype)).sum().backward()
        return y.detach(), xx.grad, w.grad, b.grad
    exp, f32 = formula(torch.float64), formula(torch.float32)
    xd = x.clone().cuda().requires_grad_()
    y = Fn.LinearFn.apply(xd, lin.weight, lin.bias, ops.ACT_SIGMOID, p, seed)
    y.backward(dy.cuda())
    ops.join_extra_streams()
    torch.cuda.synchronize()
    report = []
    for name, got, e, f in zip(('y', 'dx', 'dW', 'db'), (y.detach(), xd.grad, lin.weight.grad, lin.bias.grad), exp, f32):
        bar = _bar(e, f, name, report)
        err = float((got.cpu().double() - e).abs().max())
        report.append('kernel %s %.3e' % (name, err))
        assert err <= bar, (shape, p, name, err, bar)
    print('%s p=%s: %s' % (shape, p, '; '.join(report)))
    if p > 0:
        assert torch.equal(y.detach().cpu() == 0, ~keep)


@pytest.mark.parametrize('act', ['none', 'relu'])
def test_linear_fn_none_and_relu_are_the_same_gemm_call_as_before(act):
    """Bit-equal to a direct ops.gemm call with the arguments LinearFn has always passed."""
    from nnr_amd import ops
    from nnr_amd import functional as Fn
    M, K, N, p, seed = 67, 300, 200, 0.2, 99
    torch.manual_seed(3)
    lin = torch.nn.Linear(K, N).cuda()
    x = torch.randn(M, K).cuda()
    a = dict(none=ops.ACT_NONE, relu=ops.ACT_RELU)[act]
    y = Fn.LinearFn.apply(x, lin.weight, lin.bias, a, p, seed)
    y2 = torch.empty(M, N, device='cuda')
    r = torch.empty(M, N, device='cuda') if act == 'relu' else None
    ops.gemm(x, lin.weight, y2, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=lin.bias, act=a, aux_out=r, ldaux=N, drop=(3, p, seed, N))
    torch.cuda.synchronize()
    assert torch.equal(y.detach(), y2)


# ------------------------------------------------------------------------------------------------ the model
def _loss(model, logits):
    from nnr_amd.model import negative_log_softmax
    loss = negative_log_softmax(logits)
    if model.news_encoder.auxiliary_loss is not None:                  # trainer.py:109-114
        loss = loss + model.news_encoder.auxiliary_loss.mean()
    return loss


@pytest.mark.parametrize('tag', CASES)
def test_model_matches_reference_golden(tag):
    """The body of tests/test_hip_npa_gpu.py::test_model_matches_reference_golden with the trainer's auxiliary term, bars unchanged."""
    from nnr_amd.trainer import Trainer
    case = GoldenCase(tag)
    model, cfg = build_model(case)
    trainer = Trainer(model, cfg)
    steps = int(case.meta['adam_steps'])
    rec = {}
    ne = model.news_encoder
    ne.register_forward_hook(lambda m, i, o: rec.setdefault('reps', []).append(o.detach().cpu().numpy()))
    ue = model.user_encoder
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
        rec.pop('reps', None)
        logits = model(*batch)
        loss = _loss(model, logits)
        loss.backward()
        from nnr_amd import ops
        ops.join_extra_streams()
        torch.cuda.synchronize()
        if s == 0:
            e = {k: float(np.abs(v - case.expect(n)).max()) for k, v, n in
                 (('cand_rep', rec['reps'][0], 'cand_rep'), ('hist_rep', rec['reps'][1], 'hist_rep'), ('user_rep', rec['user'], 'user_rep'))}
            report.append('stage max-abs-err: %s' % e)
            lg = logits.detach().cpu().numpy()
            err = float(np.abs(lg - case.expect('logits')).max())
            report.append('logits err %.3e  loss err %.3e' % (err, abs(float(loss) - float(case.expect('loss')))))
            if cfg.news_encoder == 'DAE':
                aux = ne.auxiliary_loss
                assert tuple(aux.shape) == (batch[3].shape[0], batch[3].shape[1])          # the HISTORY call's [B, max_history_num]
                aerr = abs(float(aux.mean()) - float(case.expect('auxiliary_loss')))
                report.append('auxiliary_loss err %.3e' % aerr)
            else:
                assert ne.auxiliary_loss is None
                aerr = 0.0
            print('\n'.join(report))
            assert aerr <= TIGHT
            assert max(e.values()) <= TIGHT * max(1.0, float(np.abs(case.expect('hist_rep')).max())), e
            assert err <= LOGIT_TOL and err <= TIGHT * max(1.0, float(np.abs(lg).max())), err
            assert abs(float(loss) - float(case.expect('loss'))) <= TIGHT
            # in-place input mutation is part of the reference's observable behaviour (Inception: mask[:, :, 0] = 1; DAE: none)
            np.testing.assert_array_equal(batch[16].cpu().numpy(), case.expect('mutated_news_title_mask'))
            np.testing.assert_array_equal(batch[11].cpu().numpy(), case.expect('mutated_user_history_category_mask'))
            if cfg.news_encoder == 'Inception':
                assert bool(batch[16][:, :, 0].all() and batch[19][:, :, 0].all() and batch[4][:, :, 0].all() and batch[7][:, :, 0].all())
            else:
                np.testing.assert_array_equal(batch[16].cpu().numpy(), case.expect('in/news_title_mask'))
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
    # the trainer's own step takes the autograd path for these pairs and records no tape
    for _ in range(4):
        _, loss = trainer.train_step(case.batch('cuda'))
        assert trainer.last_path == 'autograd'
    assert not trainer.tapes and bool(torch.isfinite(loss))


@pytest.mark.parametrize('tag', ['tiny_DAE_ATT', 'tiny_Inception_CATT'])
def test_trainer_step_reproduces_the_reference_losses(tag):
    """Trainer.train_step itself (its own zero_grad, auxiliary term, clip and Adam): the loss of each of the three steps is the reference's."""
    from nnr_amd.trainer import Trainer
    case = GoldenCase(tag)
    model, cfg = build_model(case)
    trainer = Trainer(model, cfg)
    for s in range(int(case.meta['adam_steps'])):
        _, loss = trainer.train_step(case.batch('cuda'))
        assert trainer.last_path == 'autograd'
        assert abs(float(loss) - float(case.expect('loss_step%d' % s))) <= 5e-5, 'loss at step %d' % s


@pytest.mark.parametrize('tag', ['tiny_DAE_ATT', 'tiny_DAE_CATT'])
def test_the_history_call_wins_on_the_side_stream_branch_too(tag):
    """Model.forward issues the candidate call FIRST on a side stream when the step counts as GPU-bound (forced here by the threshold), the
    history call last: auxiliary_loss is the history call's tensor, and logits, the term and every gradient equal the sequential branch's.
    Both calls' table-gradient reductions (one plain writer per row) then come from backward nodes on two streams: they must not overlap."""
    from nnr_amd import ops
    case = GoldenCase(tag)
    runs = []
    old = ops.LEAF_MIN_ROWS
    for side in (False, True):
        model, cfg = build_model(case)
        ops.LEAF_MIN_ROWS = 1 if side else 1 << 40
        try:
            batch = case.batch('cuda')
            logits = model(*batch)
            aux = model.news_encoder.auxiliary_loss
            assert tuple(aux.shape) == tuple(batch[3].shape[:2])
            _loss(model, logits).backward()
            ops.join_extra_streams()
            torch.cuda.synchronize()
        finally:
            ops.LEAF_MIN_ROWS = old
        runs.append((logits.detach().clone(), aux.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}))
    assert abs(float(runs[1][1].mean()) - float(case.expect('auxiliary_loss'))) <= TIGHT
    assert float((runs[0][0] - runs[1][0]).abs().max()) <= 1e-6 and float((runs[0][1] - runs[1][1]).abs().max()) <= 1e-7
    total = float(case.expect('grad_total_norm'))
    for k in runs[0][2]:
        assert float((runs[0][2][k] - runs[1][2][k]).abs().max()) <= 1e-6 * max(1.0, total), k
    assert torch.equal(runs[0][2]['news_encoder.word_embedding.weight'], runs[1][2]['news_encoder.word_embedding.weight'])


@pytest.mark.parametrize('tag', TINY)
def test_plugin_calls_equal_model_forward(tag):
    case = GoldenCase(tag)
    model, cfg = build_model(case)
    logits = model(*case.batch('cuda')).detach()
    (uid, ucat, usub, utt, utm, ute, uct, ucm, uce, uhm, ug, ucmask, ucidx, ncat, nsub, ntt, ntm, nte, nct, ncm, nce) = case.batch('cuda')
    cand = model.news_encoder(ntt, ntm, nte, nct, ncm, nce, ncat, nsub, None)
    assert tuple(cand.shape) == (ntt.shape[0], ntt.shape[1], model.news_embedding_dim)
    user = model.user_encoder(utt, utm, ute, uct, ucm, uce, ucat, usub, uhm, ug, ucmask, ucidx, None, cand)
    plug = (user * cand).sum(dim=2)
    # same encoder launches on both sides; the last step differs -- Model.forward's dot-product kernel against torch's (user * cand).sum() here,
    # two summation orders of one fp32 dot product: a few ulp of the result (Inception's logits reach 29, an ulp of 1.9e-6), so 4 ulp of the
    # largest logit, and the 1e-6 of tests/test_hip_npa_gpu.py's plug-in test where that is larger
    bar = max(1e-6, 4 * 2.0 ** -23 * float(logits.abs().max()))
    err = float((plug - logits).abs().max())
    print('%s plug-in vs Model.forward %.3e (bar %.3e)' % (tag, err, bar))
    assert err <= bar
    if cfg.news_encoder == 'Inception':
        assert bool(ntm[:, :, 0].all() and ncm[:, :, 0].all() and utm[:, :, 0].all() and ucm[:, :, 0].all())     # reached the caller's tensors


@pytest.mark.parametrize('tag', ['tiny_DAE_ATT', 'tiny_Inception_ATT'])
def test_compute_scores_and_metrics_match_reference(tag):
    """evaluate.py with its news cache on (both encoders are batch-independent): every distinct news encoded once."""
    from nnr_amd import evaluate as E
    z, model = eval_fixture(tag)
    model = model.cuda().train()
    assert E.news_reps_cacheable(model)
    dc = E.dev_corpus({k: z[k] for k in z.files}, 'cuda', int(z['category_num']))
    scores = E.compute_scores(model, dc, batch_size=int(z['batch_size']))
    assert model.training and E.LAST_STATS['mode'] == 'cached'
    got = scores.cpu().numpy()
    err = float(np.abs(got - z['scores']).max())
    smax = float(np.abs(z['scores']).max())
    print('eval_%s scores max-abs-err %.3e (max |score| %.3e)' % (tag, err, smax))
    assert err <= LOGIT_TOL and err <= TIGHT * max(1.0, smax), err     # (the logits' bar of the model test, both halves: Inception's scores reach 42)
    ranks, per, mean = E.rank_metrics(scores, torch.from_numpy(z['labels']), z['sizes'])
    np.testing.assert_array_equal(ranks.cpu().numpy(), z['ranks'])
    np.testing.assert_allclose(mean.cpu().numpy(), z['metrics'], rtol=0, atol=1e-12)
    uncached = E.compute_scores(model, dc, batch_size=int(z['batch_size']), cache=False)
    derr = float((uncached - scores).abs().max())
    assert derr <= LOGIT_TOL and derr <= TIGHT * max(1.0, smax), derr


def test_dae_with_dropout_on_matches_the_restatement_fed_the_kernels_masks():
    """One DAE call in train mode at dropout 0.2, tiny size: representation, auxiliary term and every gradient of
    sum(rep * w) + aux.mean() against the float64 restatement given the kernels' own keep-masks -- the corrupted embedding (seed + 1, flat
    over [n, E]) and the two fusion sites (seed + 3 / seed + 4, flat over [n, category dim] / [n, subCategory dim])."""
    from hip_masks import flat_keep, _news_seed
    from nnr_amd import ops
    case = GoldenCase('tiny_DAE_CATT')
    p = 0.2
    model, cfg = build_model(case, dropout_rate=p)
    ne = model.news_encoder
    assert ne.training and ne.dropout_rate == p
    (uid, ucat, usub, utt, utm, ute, uct, ucm, uce, uhm, ug, ucmask, ucidx, ncat, nsub, ntt, ntm, nte, nct, ncm, nce) = case.batch('cuda')
    B, H = utt.shape[:2]
    n, E, cd, sd = B * H, int(cfg.word_embedding_dim), int(cfg.category_embedding_dim), int(cfg.subCategory_embedding_dim)
    seed = _news_seed(ne, 1)
    keep = dict(corrupt=flat_keep(n * E, p, seed + 1).view(n, E).cpu(), cat=flat_keep(n * cd, p, seed + 3).view(n, cd).cpu(),
                sub=flat_keep(n * sd, p, seed + 4).view(n, sd).cpu())
    for k, v in keep.items():
        assert 0.55 < float(v.float().mean()) < 0.97 and not bool(v.all()), k           # every site drops something
    g = torch.Generator().manual_seed(8)
    w = torch.randn(B, H, ne.news_embedding_dim, generator=g)
    for q in model.parameters():
        q.grad = None
    rep = ne(utt, utm, ute, uct, ucm, uce, ucat, usub, None)
    aux = ne.auxiliary_loss
    ((rep * w.cuda()).sum() + aux.mean()).backward()
    ops.join_extra_streams()
    torch.cuda.synchronize()
    st = {k: f64(v).requires_grad_() for k, v in model.state_dict().items() if k.startswith('news_encoder.')}
    erep, eaux, _ = bow_ref.dae_call(st, utt, utm, uct, ucm, ucat, usub, float(cfg.Alpha), p=p, keep=keep)
    ((erep * w.double()).sum() + eaux.mean()).backward()
    report = ['rep %.3e' % float((rep.detach().cpu().double() - erep.detach()).abs().max()), 'aux %.3e' % float((aux.detach().cpu().double() - eaux.detach()).abs().max())]
    assert float((rep.detach().cpu().double() - erep.detach()).abs().max()) <= TIGHT * max(1.0, float(erep.abs().max()))
    assert float((aux.detach().cpu().double() - eaux.detach()).abs().max()) <= TIGHT
    # the dropped elements are exactly the masks' (fusion columns; the corrupted embedding is internal and shows through the gradients)
    hd = int(cfg.hidden_dim)
    assert torch.equal(rep.detach().cpu().view(n, -1)[:, hd:hd + cd] == 0, ~keep['cat'] | (erep.detach().view(n, -1)[:, hd:hd + cd] == 0))
    named = dict(model.named_parameters())
    total = float(torch.sqrt(sum((v.grad ** 2).sum() for v in st.values() if v.grad is not None)))
    for k, v in st.items():
        got = named[k].grad
        exp = v.grad if v.grad is not None else torch.zeros_like(v)
        err = float(((got.cpu().double() if got is not None else torch.zeros_like(v)) - exp).abs().max())
        scale = max(1e-3, float(exp.norm()), 0.05 * total)
        report.append('d%s %.3e (bar %.3e)' % (k.split('.', 1)[1], err, 5e-5 * scale))
        assert err <= 5e-5 * scale, (k, err, scale)
    print('; '.join(report))
    assert float(st['news_encoder.f1.weight'].grad.abs().max()) > 0 and float(st['news_encoder.word_embedding.weight'].grad.abs().max()) > 0
