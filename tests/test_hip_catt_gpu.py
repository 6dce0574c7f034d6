"""The CATT user encoder and the candidate-attention layers on the GPU: the fused kernel (csrc/cand_attn.hip) against the float64
restatement of the reference's formulation (tests/cand_attn_ref.py, pinned to the reference by tests/test_catt_host.py), its
reproducibility, and the model / plugin / layer / evaluation / dropout-on paths against golden vectors captured from the reference's
own code (tests/golden/*CATT*.npz, layer_cand_attn.npz).  Bars as in tests/test_hip_model_gpu.py and tests/test_hip_eval_gpu.py."""
import os

import numpy as np
import pytest
import torch

from cand_attn_ref import pq_form, catt_user_rep, f64
from golden_io import GoldenCase, GOLDEN_DIR, build_model, eval_fixture

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4
TIGHT = 2e-5
CATT_CASES = ['tiny_CNE_CATT_stable', 'tiny_CNN_CATT', 'full_CNE_CATT_g1p0_stable']
SHAPES = [(3, 3, 6, 8, 40), (2, 5, 50, 200, 900), (64, 5, 50, 200, 900), (5, 1, 50, 200, 500), (1, 1, 1, 4, 4), (7, 4, 33, 13, 30)]
ACT_ID = {'relu': 1, 'tanh': 2}


def _inputs(B, N, H, A, D, masked, seed):
    """fp32 inputs; no pre-activation P[b,n,k] + Q[b,h,k] within 1e-4 of zero (offenders resampled), so the ReLU comparison needs no
    exclusions.  Masks: sample 0 without history, sample 1 with a full one, the others ragged."""
    g = torch.Generator().manual_seed(seed)
    P, Q = torch.randn(B, N, A, generator=g), torch.randn(B, H, A, generator=g)
    for _ in range(100):
        bad = ((P.unsqueeze(2) + Q.unsqueeze(1)).abs() < 1e-4).any(dim=1)          # [B, H, A]
        if not bool(bad.any()):
            break
        Q[bad] = torch.randn(int(bad.sum()), generator=g)
    assert float((P.unsqueeze(2) + Q.unsqueeze(1)).abs().min()) >= 1e-4
    w2 = torch.randn(A, generator=g) / A ** 0.5
    feat, dout = torch.randn(B, H, D, generator=g), torch.randn(B, N, D, generator=g)
    mask = None
    if masked:
        lens = torch.randint(0, H + 1, (B,), generator=g)
        lens[0] = 0
        if B > 1:
            lens[1] = H
        mask = torch.arange(H).unsqueeze(0) < lens.unsqueeze(1)
    return P, Q, w2, feat, dout, mask


def _expected(P, Q, w2, feat, dout, mask, act):
    p, q, w, f = (f64(t).requires_grad_() for t in (P, Q, w2, feat))
    alpha, out = pq_form(p, q, w, f, mask, act)
    (out * f64(dout)).sum().backward()
    return dict(alpha=alpha.detach(), out=out.detach(), dP=p.grad, dQ=q.grad, dw2=w.grad, dfeat=f.grad)


def _run(P, Q, w2, feat, dout, mask, act, dfeat0=None):
    from nnr_amd import ops
    B, N, A = P.shape
    H, D = feat.shape[1], feat.shape[2]
    dev = dict(device='cuda', dtype=torch.float32)
    P, Q, w2, feat, dout = (t.cuda().contiguous() for t in (P, Q, w2, feat, dout))
    mask = None if mask is None else mask.cuda().contiguous()
    alpha, out = torch.empty((B, N, H), **dev), torch.empty((B, N, D), **dev)
    ops.cand_attn_fwd(P.view(B * N, A), Q.view(B * H, A), w2, feat, mask, B, N, H, A, D, ACT_ID[act], alpha, out)
    dP, dQ, dw2 = torch.empty((B, N, A), **dev), torch.empty((B, H, A), **dev), torch.zeros(A, **dev)
    dfeat = torch.empty((B, H, D), **dev) if dfeat0 is None else dfeat0.cuda().clone()
    ops.cand_attn_bwd(P.view(B * N, A), Q.view(B * H, A), w2, feat, mask, alpha, dout, B, N, H, A, D, ACT_ID[act], dP.view(B * N, A),
                      dQ.view(B * H, A), dfeat, dw2, accumulate=dfeat0 is not None)
    torch.cuda.synchronize()
    return dict(alpha=alpha, out=out, dP=dP, dQ=dQ, dw2=dw2, dfeat=dfeat)


def _check(got, exp, tag):
    report, worst = [], {}
    for k, e in exp.items():
        err = float((got[k].cpu().double() - e).abs().max())
        emax = float(e.abs().max())
        bar = TIGHT * (emax if k in ('dw2', 'dP', 'dQ') else max(1.0, emax))      # (the score-side gradients: relative to the tensor's max)
        report.append('%s err %.3e (max|exp| %.3e, bar %.3e)' % (k, err, emax, bar))
        worst[k] = (err, bar)
    print(tag + ': ' + '; '.join(report))
    for k, (err, bar) in worst.items():
        assert err <= bar, (tag, k, err, bar)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('masked', [True, False], ids=['mask', 'nomask'])
@pytest.mark.parametrize('act', ['relu', 'tanh'])
def test_kernel_matches_the_float64_restatement(shape, masked, act):
    inp = _inputs(*shape, masked, seed=sum(shape) + 7 * masked)
    _check(_run(*inp, act), _expected(*inp, act), '%s %s %s' % (shape, 'mask' if masked else 'nomask', act))


def test_kernel_accumulates_into_a_given_feature_gradient():
    inp = _inputs(3, 3, 6, 8, 40, True, seed=5)
    base = torch.randn(3, 6, 40, generator=torch.Generator().manual_seed(9))
    exp = _expected(*inp, 'relu')
    exp['dfeat'] = exp['dfeat'] + base.double()
    _check(_run(*inp, 'relu', dfeat0=base), exp, 'accumulate')


def test_unaligned_feature_rows_take_the_scalar_path():
    """D % 4 == 0 but the feature tensor starts 4 bytes off a 16-byte boundary."""
    from nnr_amd import ops
    B, N, H, A, D = 2, 2, 5, 8, 12
    P, Q, w2, feat, dout, mask = _inputs(B, N, H, A, D, True, seed=11)
    exp = _expected(P, Q, w2, feat, dout, mask, 'relu')
    dev = dict(device='cuda', dtype=torch.float32)
    store = torch.zeros(B * H * D + 1, **dev)
    fo = store[1:].view(B, H, D)
    fo.copy_(feat)
    alpha, out = torch.empty((B, N, H), **dev), torch.empty((B, N, D), **dev)
    ops.cand_attn_fwd(P.cuda().view(B * N, A), Q.cuda().view(B * H, A), w2.cuda(), fo, mask.cuda(), B, N, H, A, D, 1, alpha, out)
    torch.cuda.synchronize()
    _check(dict(alpha=alpha, out=out), {k: exp[k] for k in ('alpha', 'out')}, 'unaligned')


def test_kernels_are_bit_reproducible():
    inp = _inputs(64, 5, 50, 200, 900, True, seed=21)
    a, b = _run(*inp, 'relu'), _run(*inp, 'relu')
    for k in ('alpha', 'out', 'dP', 'dQ', 'dfeat', 'dw2'):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('tag', CATT_CASES)
def test_model_matches_reference_golden(tag):
    """The body of tests/test_hip_model_gpu.py::test_model_matches_reference_golden, bars unchanged."""
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
            assert float(ue.affine2.bias.grad.abs().max()) == 0.0            # exactly zero (the reference's autograd leaves rounding noise)
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
    # the trainer's own step takes the autograd path for this pair and records no tape
    for _ in range(4):
        _, loss = trainer.train_step(case.batch('cuda'))
        assert trainer.last_path == 'autograd'
    assert not trainer.tapes and bool(torch.isfinite(loss))


@pytest.mark.parametrize('tag', ['tiny_CNE_CATT_stable', 'full_CNE_CATT_g1p0_stable'])
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


@pytest.mark.parametrize('kind', ['single', 'multi'])
@pytest.mark.parametrize('mtag', ['mask', 'nomask'])
def test_layers_match_the_reference(kind, mtag):
    from nnr_amd.layers import CandidateAttention, MultipleCandidateAttention
    z = np.load(os.path.join(GOLDEN_DIR, 'layer_cand_attn.npz'))
    mod = (CandidateAttention if kind == 'single' else MultipleCandidateAttention)(24, 24, 12)
    assert list(mod.state_dict().keys()) == [str(k) for k in z[kind + '/param_names']]
    mod.load_state_dict({str(k): torch.from_numpy(z['%s/param/%s' % (kind, k)].copy()) for k in z[kind + '/param_names']})
    mod = mod.cuda()
    feat = torch.from_numpy(z['feature'].copy()).cuda().requires_grad_()
    query = torch.from_numpy(z[kind + '/query'].copy()).cuda().requires_grad_()
    mask = torch.from_numpy(z['mask'].copy()).cuda() if mtag == 'mask' else None
    out = mod(feat, query, mask)
    out.square().sum().backward()
    torch.cuda.synchronize()
    pre = '%s/%s/' % (kind, mtag)
    assert tuple(out.shape) == tuple(z[pre + 'out'].shape)
    assert float(np.abs(out.detach().cpu().numpy() - z[pre + 'out']).max()) <= 2e-5
    got = {'feature': feat.grad, 'query': query.grad}
    got.update({'param/' + k: p.grad for k, p in mod.named_parameters()})
    for k, g in got.items():
        e = z[pre + 'grad/' + k]
        err = float(np.abs(g.cpu().numpy() - e).max())
        print('%s%s err %.3e' % (pre, k, err))
        assert err <= 5e-5 * max(1e-3, float(np.linalg.norm(e.astype(np.float64)))), k


def _eval_model(tag):
    z, model = eval_fixture(tag)
    return z, model.cuda().train()


@pytest.mark.parametrize('tag', ['tiny_CNN_CATT', 'tiny_CNE_CATT_stable'])
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
    z, model = _eval_model('tiny_CNN_CATT')
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


def test_cne_catt_still_refuses_caching():
    from nnr_amd import evaluate as E
    z, model = _eval_model('tiny_CNE_CATT_stable')
    assert not E.news_reps_cacheable(model)
    dc = E.dev_corpus({k: z[k] for k in z.files}, 'cuda', int(z['category_num']))
    scores = E.compute_scores(model, dc, batch_size=8)                    # 'auto' -> per-sample
    assert E.LAST_STATS['mode'] == 'per-sample'
    assert float(np.abs(scores.cpu().numpy() - z['scores']).max()) <= 2e-5


def test_dropout_on_training_steps_feed_catt_what_the_news_encoder_produced():
    """CNE + CATT at the 200k defaults (dropout 0.2), batch 8: two steps on the same batch draw different masks, and the CATT stage
    (which has no dropout site of its own) turns the recorded history / candidate representations of that very run into the
    restatement's user representation."""
    from nnr_amd.config import make_config
    from nnr_amd.model import Model
    from nnr_amd.synth import SynthSpec, SynthCorpus, to_torch
    from nnr_amd.trainer import Trainer
    cfg = make_config(['--news_encoder=CNE', '--user_encoder=CATT', '--batch_size=8'], corpus_sizes=dict(vocabulary_size=2000))
    assert cfg.dropout_rate == 0.2
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
        rec[-1].update(user=o.detach().clone(), mask=a[1].clone(), state={'user_encoder.' + k: v.detach().clone() for k, v in ue.state_dict().items()
                                                                         if not k.startswith('news_encoder.')})
        return o
    ne.forward_pair, ue.encode_user = recording_pair, recording_enc
    outs = []
    for _ in range(2):
        logits, loss = trainer.train_step(to_torch(batch, 'cuda'))
        torch.cuda.synchronize()
        assert trainer.last_path == 'autograd' and bool(torch.isfinite(loss))
        outs.append(logits.clone())
    assert float((outs[0] - outs[1]).abs().max()) > 1e-4                  # the second step drew other dropout masks
    for r in rec:
        exp = catt_user_rep(r['hist'], r['cand'], r['mask'], {k: v.cpu().numpy() for k, v in r['state'].items()})
        err = float((r['user'].cpu().double() - exp).abs().max())
        print('CATT stage vs restatement %.3e (max|exp| %.3e)' % (err, float(exp.abs().max())))
        assert err <= TIGHT * max(1.0, float(exp.abs().max()))
