"""NPA on the GPU: the per-title personalised attention kernel (csrc/pers_attn.hip) and the user-row kernels (csrc/misc.hip) against the
float64 restatements of tests/npa_ref.py (pinned to the reference by tests/test_npa_host.py), their guards and reproducibility, and the
PNE / PUE model, plug-in, evaluation and dropout-on paths against golden vectors captured from the reference's own code
(tests/golden/*PNE*.npz, *PUE*.npz).  Bars as in tests/test_hip_catt_gpu.py."""

import numpy as np
import pytest
import torch

from golden_io import GoldenCase, build_model, eval_fixture
from npa_ref import pers_attn, pne_title_rep, pue_user_rep, f64

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4
TIGHT = 2e-5
NPA_CASES = ['tiny_PNE_PUE', 'tiny_PNE_ATT', 'tiny_CNN_PUE', 'full_PNE_PUE_g1p0']
# (n, L, A, F, U): the degenerate case | a partial last workgroup, A and F no multiples of 4, several titles per user | L above 32 | the L cap |
# the product's dimensions
SHAPES = [(1, 1, 4, 4, 1), (5, 7, 13, 30, 3), (4, 33, 8, 12, 2), (6, 64, 200, 400, 6), (9, 32, 200, 400, 4)]
UNSUPPORTED = -3


def _inputs(n, Lx, A, F, U, masked, seed, sparse_users=False):
    """fp32 inputs.  Masks: title 0 all-masked, title 1 all-live, the others random bit patterns (holes, not prefixes) with at least one
    live position.  Index map: arange(n) % U, or with `sparse_users` arange(n) % (U - 1), which leaves user U - 1 without titles."""
    g = torch.Generator().manual_seed(seed)
    Qf, P = torch.randn(n, Lx, A, generator=g), torch.randn(U, A, generator=g)
    w2 = torch.randn(A, generator=g) / A ** 0.5
    feat, dout = torch.randn(n, Lx, F, generator=g), torch.randn(n, F, generator=g)
    uidx = (torch.arange(n) % (U - 1 if sparse_users else U)).to(torch.int32)
    mask = None
    if masked:
        mask = torch.rand(n, Lx, generator=g) < 0.45
        mask[torch.arange(n), torch.randint(0, Lx, (n,), generator=g)] = True
        mask[0] = False
        if n > 1:
            mask[1] = True
    return Qf, P, uidx, w2, feat, dout, mask


def _expected(Qf, P, uidx, w2, feat, dout, mask):
    q, p, w, f = (f64(t).requires_grad_() for t in (Qf, P, w2, feat))
    alpha, out = pers_attn(q, p, uidx, w, f, mask)
    (out * f64(dout)).sum().backward()
    return dict(alpha=alpha.detach(), out=out.detach(), dP=p.grad, dQf=q.grad, dw2=w.grad, dfeat=f.grad)


def _run(Qf, P, uidx, w2, feat, dout, mask, feat_dev=None):
    from nnr_amd import ops
    n, Lx, A = Qf.shape
    F, U = feat.shape[2], P.shape[0]
    dev = dict(device='cuda', dtype=torch.float32)
    Qf, P, w2, dout, uidx = (t.cuda().contiguous() for t in (Qf, P, w2, dout, uidx))
    feat = feat.cuda().contiguous() if feat_dev is None else feat_dev
    mask = None if mask is None else mask.cuda().contiguous()
    alpha, out = torch.empty((n, Lx), **dev), torch.empty((n, F), **dev)
    rc = ops.pers_attn_fwd(Qf.view(n * Lx, A), P, uidx, w2, feat, mask, n, Lx, A, F, alpha, out)
    assert rc == 0, rc
    dP, dQf, dw2, dfeat = torch.empty((U, A), **dev), torch.empty((n, Lx, A), **dev), torch.zeros(A, **dev), torch.empty((n, Lx, F), **dev)
    ops.pers_attn_bwd(Qf.view(n * Lx, A), P, uidx, w2, feat, mask, alpha, dout, n, Lx, A, F, dP, dQf.view(n * Lx, A), dfeat, dw2)
    torch.cuda.synchronize()
    return dict(alpha=alpha, out=out, dP=dP, dQf=dQf, dw2=dw2, dfeat=dfeat)


def _check(got, exp, tag):
    report, worst = [], {}
    for k, e in exp.items():
        err = float((got[k].cpu().double() - e).abs().max())
        emax = float(e.abs().max())
        bar = TIGHT * (emax if k in ('dw2', 'dP', 'dQf') else max(1.0, emax))      # (the score-side gradients: relative to the tensor's max)
        report.append('%s err %.3e (max|exp| %.3e, bar %.3e)' % (k, err, emax, bar))
        worst[k] = (err, bar)
    print(tag + ': ' + '; '.join(report))
    for k, (err, bar) in worst.items():
        assert err <= bar, (tag, k, err, bar)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('masked', [True, False], ids=['mask', 'nomask'])
def test_kernel_matches_the_float64_restatement(shape, masked):
    inp = _inputs(*shape, masked, seed=sum(shape) + 7 * masked)
    got = _run(*inp)
    _check(got, _expected(*inp), '%s %s' % (shape, 'mask' if masked else 'nomask'))
    if masked:
        assert float(got['dQf'][0].abs().max()) == 0.0                          # an all-masked title passes no gradient to its scores
        assert float((got['alpha'][0] - 1.0 / shape[1]).abs().max()) <= 1e-7


@pytest.mark.parametrize('shape', [s for s in SHAPES if s[4] >= 2], ids=lambda s: 'x'.join(map(str, s)))
def test_a_user_without_titles_gets_an_exactly_zero_row(shape):
    inp = _inputs(*shape, True, seed=sum(shape) + 3, sparse_users=True)
    got = _run(*inp)
    _check(got, _expected(*inp), '%s sparse users' % (shape,))
    assert float(got['dP'][shape[4] - 1].abs().max()) == 0.0


def _layer(Fd, Qd, A, seed):
    from nnr_amd.layers import CandidateAttention
    torch.manual_seed(seed)
    mod = CandidateAttention(Fd, Qd, A)
    mod.initialize()
    with torch.no_grad():
        mod.query_affine.bias.uniform_(-0.5, 0.5)
    return mod


def test_a_shape_beyond_the_limit_is_unsupported_and_the_layer_falls_back():
    """L = 65 is one past the one-score-per-lane limit: the entry point says NNR_ERR_UNSUPPORTED, and layers.personalized_attention runs the
    candidate-attention kernels on the query rows expanded through uidx -- same result, same bars."""
    from nnr_amd import ops
    from nnr_amd.layers import personalized_attention
    n, Lx, A, F, U, Qd = 5, 65, 8, 12, 2, 6
    Qf, P, uidx, w2, feat, dout, mask = _inputs(n, Lx, A, F, U, True, seed=17)
    dev = dict(device='cuda', dtype=torch.float32)
    alpha, out = torch.empty((n, Lx), **dev), torch.empty((n, F), **dev)
    assert ops.pers_attn_fwd(Qf.cuda().view(n * Lx, A), P.cuda(), uidx.cuda(), w2.cuda(), feat.cuda(), mask.cuda(), n, Lx, A, F, alpha, out) == UNSUPPORTED
    mod = _layer(F, Qd, A, 3)
    query = torch.randn(U, Qd, generator=torch.Generator().manual_seed(4))
    st = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    f, q = f64(feat).requires_grad_(), f64(query).requires_grad_()
    par = {k: f64(v).requires_grad_() for k, v in st.items()}
    _, eo = pers_attn(f @ par['feature_affine.weight'].t(), q @ par['query_affine.weight'].t() + par['query_affine.bias'], uidx,
                      par['attention_affine.weight'].reshape(-1), f, mask)
    (eo * f64(dout)).sum().backward()
    mod = mod.cuda()
    fg, qg = feat.cuda().requires_grad_(), query.cuda().requires_grad_()
    go = personalized_attention(mod, fg, qg, uidx.cuda(), mask.cuda())
    (go * dout.cuda()).sum().backward()
    torch.cuda.synchronize()
    got = dict(out=go.detach(), dfeat=fg.grad, dquery=qg.grad)
    exp = dict(out=eo.detach(), dfeat=f.grad, dquery=q.grad)
    for k, p in mod.named_parameters():
        got['d' + k], exp['d' + k] = p.grad, par[k].grad
    for k, e in exp.items():
        err, emax = float((got[k].cpu().double() - e).abs().max()), float(e.abs().max())
        print('fallback %s err %.3e (max|exp| %.3e)' % (k, err, emax))
        assert err <= TIGHT * max(1.0, emax), k


def test_the_layer_function_matches_the_restatement_through_the_kernel():
    """layers._PersAttnFn end to end (projection GEMMs, kernel, parameter gradients) at a supported shape: the same comparison as the fallback's."""
    from nnr_amd.layers import _PersAttnFn
    n, Lx, A, F, U, Qd = 7, 9, 8, 12, 3, 6
    Qf, P, uidx, w2, feat, dout, mask = _inputs(n, Lx, A, F, U, True, seed=23)
    mod = _layer(F, Qd, A, 5)
    query = torch.randn(U, Qd, generator=torch.Generator().manual_seed(6))
    f, q = f64(feat).requires_grad_(), f64(query).requires_grad_()
    par = {k: f64(v).requires_grad_() for k, v in mod.state_dict().items()}
    _, eo = pers_attn(f @ par['feature_affine.weight'].t(), q @ par['query_affine.weight'].t() + par['query_affine.bias'], uidx,
                      par['attention_affine.weight'].reshape(-1), f, mask)
    (eo * f64(dout)).sum().backward()
    mod = mod.cuda()
    fg, qg = feat.cuda().requires_grad_(), query.cuda().requires_grad_()
    go = _PersAttnFn.apply(fg, qg, uidx.cuda(), mod, mask.cuda())
    (go * dout.cuda()).sum().backward()
    torch.cuda.synchronize()
    got = dict(out=go.detach(), dfeat=fg.grad, dquery=qg.grad)
    exp = dict(out=eo.detach(), dfeat=f.grad, dquery=q.grad)
    for k, p in mod.named_parameters():
        got['d' + k], exp['d' + k] = p.grad, par[k].grad
    for k, e in exp.items():
        err, emax = float((got[k].cpu().double() - e).abs().max()), float(e.abs().max())
        print('layer %s err %.3e (max|exp| %.3e)' % (k, err, emax))
        assert err <= TIGHT * max(1.0, emax), k


def test_unaligned_feature_rows_take_the_scalar_path():
    """A % 4 == F % 4 == 0 but the feature tensor starts 4 bytes off a 16-byte boundary."""
    n, Lx, A, F, U = 5, 6, 8, 12, 2
    inp = _inputs(n, Lx, A, F, U, True, seed=11)
    store = torch.zeros(n * Lx * F + 1, device='cuda', dtype=torch.float32)
    fo = store[1:].view(n, Lx, F)
    fo.copy_(inp[4])
    assert fo.data_ptr() % 16 == 4
    _check(_run(*inp, feat_dev=fo), _expected(*inp), 'unaligned')


def test_kernels_are_bit_reproducible():
    inp = _inputs(320, 32, 200, 400, 64, True, seed=21)
    a, b = _run(*inp), _run(*inp)
    for k in ('alpha', 'out', 'dP', 'dQf', 'dfeat', 'dw2'):
        assert torch.equal(a[k], b[k]), k


def test_an_out_of_range_index_means_no_query_and_touches_nothing_outside():
    """uidx holds U + 1 while P / dP are ALLOCATED with U + 3 rows: the title attends with P = 0, and dP's rows from U on keep their sentinel."""
    from nnr_amd import ops
    n, Lx, A, F, U, extra = 6, 7, 8, 12, 3, 3
    Qf, P, uidx, w2, feat, dout, mask = _inputs(n, Lx, A, F, U, True, seed=31)
    uidx[3] = U + 1
    uidx[4] = -2
    exp = _expected(Qf, P, uidx, w2, feat, dout, mask)
    dev = dict(device='cuda', dtype=torch.float32)
    Pbig = torch.cat([P, torch.full((extra, A), 1e3)]).cuda()                   # (what a read past U would pick up)
    dPbig = torch.full((U + extra, A), 777.0, **dev)
    Qd, w2d, fd, dd, ud, md = Qf.cuda().view(n * Lx, A), w2.cuda(), feat.cuda(), dout.cuda(), uidx.cuda(), mask.cuda()
    alpha, out = torch.empty((n, Lx), **dev), torch.empty((n, F), **dev)
    assert ops.pers_attn_fwd(Qd, Pbig, ud, w2d, fd, md, n, Lx, A, F, alpha, out, U=U) == 0
    dQf, dw2, dfeat = torch.empty((n * Lx, A), **dev), torch.zeros(A, **dev), torch.empty((n, Lx, F), **dev)
    ops.pers_attn_bwd(Qd, Pbig, ud, w2d, fd, md, alpha, dd, n, Lx, A, F, dPbig, dQf, dfeat, dw2, U=U)
    torch.cuda.synchronize()
    assert float((dPbig[U:] - 777.0).abs().max()) == 0.0
    _check(dict(alpha=alpha, out=out, dP=dPbig[:U], dQf=dQf.view(n, Lx, A), dw2=dw2, dfeat=dfeat), exp, 'out-of-range uidx')


# ------------------------------------------------------------------------------------------------ user rows
def test_user_rows_forward_is_a_gather_and_guards_the_id():
    from nnr_amd import ops
    g = torch.Generator().manual_seed(1)
    table = torch.randn(8, 6, generator=g).cuda()
    ids = torch.tensor([3, 0, 4, 3, 1], dtype=torch.int64).cuda()
    assert torch.equal(ops.user_rows_fwd(table, ids, 0.0, 5), table[ids])
    # an 8-row allocation passed as a 5-row table, one id of 6: a zero row forward, no gradient, rows 5..7 untouched
    bad = torch.tensor([3, 6, 4, -1, 1], dtype=torch.int64).cuda()
    out = ops.user_rows_fwd(table, bad, 0.0, 5, rows=5)
    assert float(out[1].abs().max()) == 0.0 and float(out[3].abs().max()) == 0.0
    assert torch.equal(out[[0, 2, 4]], table[bad[[0, 2, 4]]])
    dtable = torch.full((8, 6), 9.0, device='cuda')
    dout = torch.randn(5, 6, generator=g).cuda()
    ops.user_rows_bwd(dout, bad, dtable, 0.0, 5, rows=5)
    torch.cuda.synchronize()
    assert float((dtable[5:] - 9.0).abs().max()) == 0.0 and float((dtable[[0, 2]] - 9.0).abs().max()) == 0.0
    assert torch.equal(dtable[[3, 4, 1]], 9.0 + dout[[0, 2, 4]])


def test_user_rows_backward_applies_the_forward_mask_and_sums_duplicates_in_order():
    from nnr_amd import ops
    g = torch.Generator().manual_seed(2)
    rows, dim, B, p, seed = 9, 50, 64, 0.2, 12345
    table = (torch.rand(rows, dim, generator=g) + 0.5).cuda()                    # (no zero entry: the forward output shows the mask)
    uniq = torch.tensor([5, 0, 7, 2], dtype=torch.int64).cuda()
    fwd = ops.user_rows_fwd(table, uniq, p, seed)
    keep = fwd != 0
    assert 0.6 < float(keep.float().mean()) < 0.95
    assert float((fwd[keep] - (table[uniq] / (1 - p))[keep]).abs().max()) <= 1e-6
    dtable = torch.zeros(rows, dim, device='cuda')
    ops.user_rows_bwd(torch.ones(4, dim, device='cuda'), uniq, dtable, p, seed)
    assert torch.equal(dtable[uniq] != 0, keep) and float((dtable[uniq][keep] - 1 / (1 - p)).abs().max()) <= 1e-6
    # duplicates: 64 rows over 9 ids (id 0 among them); two runs give the same bits, and the sum is the masked rows' in fp32
    ids = torch.randint(0, rows, (B,), generator=g).cuda()
    dout = torch.randn(B, dim, generator=g).cuda()
    mask = ops.user_rows_fwd(torch.ones(rows, dim, device='cuda'), ids, p, seed)   # = keep / (1 - p)
    runs = []
    for _ in range(2):
        dt = torch.zeros(rows, dim, device='cuda')
        ops.user_rows_bwd(dout, ids, dt, p, seed)
        runs.append(dt)
    torch.cuda.synchronize()
    assert torch.equal(runs[0], runs[1])
    exp = torch.zeros(rows, dim, dtype=torch.float64).index_add_(0, ids.cpu(), (dout * mask).cpu().double())
    assert float((runs[0].cpu().double() - exp).abs().max()) <= 1e-6 * max(1.0, float(exp.abs().max()))


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize('tag', NPA_CASES)
def test_model_matches_reference_golden(tag):
    """The body of tests/test_hip_catt_gpu.py::test_model_matches_reference_golden, bars unchanged."""
    from nnr_amd.trainer import Trainer
    from nnr_amd.model import negative_log_softmax
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
            assert 'user_embedding.weight' in dict(model.named_parameters())
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


@pytest.mark.parametrize('tag', ['tiny_PNE_PUE', 'tiny_PNE_ATT', 'tiny_CNN_PUE'])
def test_plugin_calls_equal_model_forward(tag):
    case = GoldenCase(tag)
    model, cfg = build_model(case)
    logits = model(*case.batch('cuda')).detach()
    b = case.batch('cuda')
    (uid, ucat, usub, utt, utm, ute, uct, ucm, uce, uhm, ug, ucmask, ucidx, ncat, nsub, ntt, ntm, nte, nct, ncm, nce) = b
    rows = model.user_rows(uid)
    assert tuple(rows.shape) == (uid.shape[0], int(cfg.user_embedding_dim))
    cand = model.news_encoder(ntt, ntm, nte, nct, ncm, nce, ncat, nsub, rows)
    user = model.user_encoder(utt, utm, ute, uct, ucm, uce, ucat, usub, uhm, ug, ucmask, ucidx, rows, cand)
    assert tuple(user.shape) == tuple(cand.shape)
    plug = (user * cand).sum(dim=2)
    assert float((plug - logits).abs().max()) <= 1e-6


def test_compute_scores_and_metrics_match_reference():
    from nnr_amd import evaluate as E
    z, model = eval_fixture('tiny_PNE_PUE')
    model = model.cuda().train()
    assert not E.news_reps_cacheable(model)
    dc = E.dev_corpus({k: z[k] for k in z.files}, 'cuda', int(z['category_num']))
    scores = E.compute_scores(model, dc, batch_size=int(z['batch_size']))          # 'auto' -> per-sample; PNE's scores depend on the batch size
    assert model.training and E.LAST_STATS['mode'] == 'per-sample'
    got = scores.cpu().numpy()
    err = float(np.abs(got - z['scores']).max())
    print('eval_tiny_PNE_PUE scores max-abs-err %.3e' % err)
    assert err <= 2e-5, err
    ranks, per, mean = E.rank_metrics(scores, torch.from_numpy(z['labels']), z['sizes'])
    np.testing.assert_array_equal(ranks.cpu().numpy(), z['ranks'])
    np.testing.assert_allclose(mean.cpu().numpy(), z['metrics'], rtol=0, atol=1e-12)


def test_dropout_on_training_steps_feed_the_personalised_stages_what_the_run_produced():
    """PNE + PUE at the 200k defaults (dropout 0.2), batch 8: two steps on the same batch draw different masks, and the PNE pooling stage and
    the PUE stage (neither has a dropout site of its own) turn the user rows, conv outputs and history representations recorded in that
    very run into the restatements' results."""
    from nnr_amd.config import make_config
    from nnr_amd.model import Model
    from nnr_amd import news_encoders as NE
    from nnr_amd.synth import SynthSpec, SynthCorpus, to_torch
    from nnr_amd.trainer import Trainer
    cfg = make_config(['--news_encoder=PNE', '--user_encoder=PUE', '--batch_size=8'], corpus_sizes=dict(vocabulary_size=2000, user_num=8))
    assert cfg.dropout_rate == 0.2
    torch.manual_seed(0)
    model = Model(cfg)
    model.initialize()
    model = model.cuda().train()
    trainer = Trainer(model, cfg)
    batch = SynthCorpus(SynthSpec(vocabulary_size=cfg.vocabulary_size, news_pool=400, seed=3)).batch(8, np.random.default_rng(5))
    rec = []
    ue = model.user_encoder
    orig_rows, orig_pool, orig_enc = model.user_rows, NE.personalized_attention, ue.encode_user

    def recording_rows(uid):
        o = orig_rows(uid)
        rec.append(dict(rows=o.detach().clone(), pools=[]))
        return o

    def recording_pool(mod, feature, query, uidx, mask=None):
        o = orig_pool(mod, feature, query, uidx, mask)
        rec[-1]['pools'].append(dict(c=feature.detach().clone(), mask=mask.clone(), rep=o.detach().clone()))
        return o

    def recording_enc(*a):
        o = orig_enc(*a)
        rec[-1].update(user=o.detach().clone(), hist=a[0].detach().clone(), hmask=a[1].clone(),
                       state={k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
        return o
    model.user_rows, NE.personalized_attention, ue.encode_user = recording_rows, recording_pool, recording_enc
    try:
        outs = []
        for _ in range(2):
            logits, loss = trainer.train_step(to_torch(batch, 'cuda'))
            torch.cuda.synchronize()
            assert trainer.last_path == 'autograd' and bool(torch.isfinite(loss))
            outs.append(logits.clone())
    finally:
        NE.personalized_attention = orig_pool
    assert float((outs[0] - outs[1]).abs().max()) > 1e-4                  # the second step drew other dropout masks
    assert len(rec) == 2 and float((rec[0]['rows'] - rec[1]['rows']).abs().max()) > 0
    for r in rec:
        assert len(r['pools']) == 2
        for pool, news_num in zip(r['pools'], (1 + cfg.negative_sample_num, cfg.max_history_num)):
            exp = pne_title_rep(pool['c'], r['rows'], r['state'], 8, news_num, mask=pool['mask'])
            err = float((pool['rep'].cpu().double() - exp).abs().max())
            print('PNE pooling stage vs restatement %.3e (max|exp| %.3e)' % (err, float(exp.abs().max())))
            assert err <= TIGHT * max(1.0, float(exp.abs().max()))
        exp = pue_user_rep(r['hist'], r['rows'], r['hmask'], r['state'])
        err = float((r['user'][:, 0].cpu().double() - exp).abs().max())
        print('PUE stage vs restatement %.3e (max|exp| %.3e)' % (err, float(exp.abs().max())))
        assert err <= TIGHT * max(1.0, float(exp.abs().max()))
