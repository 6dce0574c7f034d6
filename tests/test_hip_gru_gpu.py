"""The GRU user encoder on the GPU: the recurrence kernels (csrc/gru.hip) against the float64 restatement tests/gru_ref.py (pinned to
torch.nn.GRU on a PackedSequence by tests/test_gru_host.py), the pack kernel against its host mirror, reproducibility, and the model /
plugin / evaluation paths against golden vectors captured from the reference's own code (tests/golden/*GRU*.npz).  Bars: h within 2e-5
absolute, every gradient within 5e-5 of its own largest magnitude (the house bars of tests/test_hip_catt_gpu.py; torch's own fp32 GRU stays
within 7e-7 / 6e-7 of float64 at (64, 50, 300, 200)); model level as tests/test_hip_catt_gpu.py::test_model_matches_reference_golden."""
import functools

import numpy as np
import pytest
import torch

import gru_ref
from golden_io import GoldenCase, build_model, eval_fixture

pytestmark = pytest.mark.gpu

H_TOL = 2e-5
G_TOL = 5e-5
LOGIT_TOL = 1e-4
TIGHT = 2e-5
# (B, T, D, H, lengths or None = random with an empty and a full user)
SHAPES = {
    'partial_tile': (5, 7, 12, 10, [7, 0, 3, 1, 7]),          # H below one MFMA block
    'second_tile': (19, 50, 100, 48, None),                   # second tile of 3 rows, full T
    'three_tiles': (33, 9, 20, 112, None),
    'product': (16, 50, 300, 200, None),                      # the product's shape
    'all_empty': (3, 4, 6, 20, [0, 0, 0]),
}
MODEL_CASES = ['tiny_DAE_GRU', 'tiny_CNN_GRU', 'tiny_CNE_GRU_h48', 'full_DAE_GRU_g1p0']
NAMES = ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')


@functools.lru_cache(maxsize=None)
def _problem(name, with_h0=False, scatter=False):
    """fp32 inputs of a shape and the float64 results (computed once, shared, never modified)."""
    B, T, D, H, lens = SHAPES[name]
    g = torch.Generator().manual_seed(B * 131 + T * 7 + H)
    k = 1.0 / H ** 0.5
    p = [torch.empty(s).uniform_(-k, k, generator=g) for s in ((3 * H, D), (3 * H, H), (3 * H,), (3 * H,))]
    x = torch.randn(B, T, D, generator=g)
    if lens is None:
        lens = torch.randint(0, T + 1, (B,), generator=g)
        lens[0], lens[1] = 0, T
    lens = torch.as_tensor(lens)
    mask = gru_ref.prefix_mask(lens, T)
    if scatter:                                                 # ones that are not a prefix: only their count matters
        mask = torch.stack([row[torch.randperm(T, generator=g)] for row in mask])
    h0 = torch.randn(B, H, generator=g) if with_h0 else None
    dout = torch.randn(B, H, generator=g)
    leaves = [gru_ref.f64(t).requires_grad_() for t in [x] + p + ([h0] if with_h0 else [])]
    hs, hf = gru_ref.gru_frozen(leaves[0], gru_ref.lengths(mask), *leaves[1:5], h0=leaves[5] if with_h0 else None)
    (hf * gru_ref.f64(dout)).sum().backward()
    exp = dict(hfinal=hf.detach(), hs=hs.detach(), dx=leaves[0].grad, lens=lens)
    exp.update({'d' + n: t.grad for n, t in zip(NAMES, leaves[1:5])})
    if with_h0:
        exp['dh0'] = leaves[5].grad
    return dict(x=x, p=p, mask=mask, h0=h0, dout=dout, dims=(B, T, D, H)), exp


def _run(inp):
    from nnr_amd import functional as Fn
    from nnr_amd.layers import GRUParams
    B, T, D, H = inp['dims']
    gru = GRUParams(D, H)
    with torch.no_grad():
        for n, t in zip(NAMES, inp['p']):
            getattr(gru, n).copy_(t)
    gru = gru.cuda()
    x = inp['x'].cuda().requires_grad_()
    h0 = inp['h0'].cuda().requires_grad_() if inp['h0'] is not None else None
    hf, length, hs = Fn.GruFn.apply(x, inp['mask'].cuda(), gru, h0)
    (hf * inp['dout'].cuda()).sum().backward()
    torch.cuda.synchronize()
    got = dict(hfinal=hf.detach(), hs=hs, dx=x.grad, lens=length)
    got.update({'d' + n: getattr(gru, n).grad for n in NAMES})
    if h0 is not None:
        got['dh0'] = h0.grad
    return got


def _check(got, exp, tag):
    report, bad = [], []
    assert torch.equal(got['lens'].cpu().long(), exp['lens'].long()), tag
    for k, e in exp.items():
        if k == 'lens':
            continue
        g = got[k].cpu().double()
        assert bool(torch.isfinite(g).all()), (tag, k)
        err, emax = float((g - e).abs().max()), float(e.abs().max())
        bar = H_TOL if k in ('hfinal', 'hs') else G_TOL * emax
        report.append('%s err %.3e (max|exp| %.3e, bar %.3e)' % (k, err, emax, bar))
        if err > bar:
            bad.append((k, err, bar))
    print(tag + ': ' + '; '.join(report))
    assert not bad, (tag, bad)


@pytest.mark.parametrize('name', list(SHAPES))
def test_kernels_match_the_float64_restatement(name):
    inp, exp = _problem(name)
    _check(_run(inp), exp, name)


def test_all_empty_batch_is_exactly_zero():
    inp, exp = _problem('all_empty')
    got = _run(inp)
    for k, v in got.items():
        if k != 'lens':
            assert float(v.abs().max()) == 0.0 and bool(torch.isfinite(v).all()), k


def test_only_the_count_of_mask_ones_matters():
    """[0, 1, 1, 0, ...] runs history slots 0 and 1."""
    inp, exp = _problem('partial_tile', scatter=True)
    assert not torch.equal(inp['mask'], gru_ref.prefix_mask(exp['lens'], inp['dims'][1]))
    _check(_run(inp), exp, 'scattered mask')
    base, _ = _problem('partial_tile')
    m = torch.zeros(5, 7, dtype=torch.bool)
    m[:, 1:3] = True
    a = _run(dict(base, mask=m))
    b = _run(dict(base, mask=gru_ref.prefix_mask([2] * 5, 7)))
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('name', ['partial_tile', 'second_tile'])
def test_start_state_and_its_gradient(name):
    """h0 given: a user without history returns h0[b] and passes dh straight to dh0."""
    inp, exp = _problem(name, with_h0=True)
    got = _run(inp)
    _check(got, exp, name + ' h0')
    empty = exp['lens'] == 0
    assert bool(empty.any())
    assert torch.equal(got['hfinal'].cpu()[empty], inp['h0'][empty]) and torch.equal(got['dh0'].cpu()[empty], inp['dout'][empty])


@pytest.mark.parametrize('H,D', [(10, 12), (48, 100), (200, 300), (256, 8), (17, 5)])
def test_pack_kernel_equals_the_host_mirror_bit_for_bit(H, D):
    from nnr_amd import ops
    g = torch.Generator().manual_seed(H + D)
    p = [torch.randn(s, generator=g) for s in ((3 * H, D), (3 * H, H), (3 * H,), (3 * H,))]
    w = ops.GruPacked([t.cuda() for t in p], H, D)
    torch.cuda.synchronize()
    for name, e in zip(('w_ihp', 'b_p', 'wf', 'wb'), ops.gru_pack_host(*p)):
        assert torch.equal(getattr(w, name).cpu(), e), name


def test_two_runs_give_identical_bits():
    inp, _ = _problem('product')
    a, b = _run(inp), _run(inp)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    inp, _ = _problem('three_tiles')                           # (H = 112, D = 20: the weight gradients' reductions take other tiles)
    a, b = _run(inp), _run(inp)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_unsupported_sizes_return_the_error_code():
    from nnr_amd import ops, _lib
    x = torch.zeros(64, device='cuda')
    with pytest.raises(_lib.NnrHipError):
        ops.gru_dims(257)
    lib = _lib.lib()
    n = torch.zeros(4, dtype=torch.int32, device='cuda')
    assert lib.nnr_gru_fwd(x.data_ptr(), x.data_ptr(), None, x.data_ptr(), 1, 256, 8, x.data_ptr(), x.data_ptr(), x.data_ptr(), n.data_ptr(), None) != 0
    assert lib.nnr_gru_bwd(x.data_ptr(), n.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 4, 300, None, None) != 0


# ---------------------------------------------------------------------------------------------- model level
@pytest.mark.parametrize('tag', MODEL_CASES)
def test_model_matches_reference_golden(tag):
    """The body of tests/test_hip_catt_gpu.py::test_model_matches_reference_golden, bars unchanged; plus: the user vectors of the users
    without history are exactly zero, and the restatement on the recorded history representation gives the recorded user representation."""
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
        state0 = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()} if s == 0 else None
        trainer.flat.zero_grad()
        logits = model(*batch)
        loss = negative_log_softmax(logits)
        if getattr(ne, 'auxiliary_loss', None) is not None:      # trainer.py:109-114 (DAE's reconstruction term)
            loss = loss + ne.auxiliary_loss.mean()
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
            lens = case.expect('in/user_history_mask').astype(bool).sum(axis=1)
            assert float(np.abs(rec['user'][lens == 0]).max(initial=0.0)) == 0.0          # exactly zero, not tanh(dec.bias)
            stage = gru_ref.gru_user_rep(rec['reps'][1], case.expect('in/user_history_mask'), state0).unsqueeze(1)
            assert float((torch.from_numpy(rec['user']).double() - stage).abs().max()) <= TIGHT
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
    # the trainer's own step takes the autograd path for this pair and records no tape
    for _ in range(4):
        _, loss = trainer.train_step(case.batch('cuda'))
        assert trainer.last_path == 'autograd'
    assert not trainer.tapes and bool(torch.isfinite(loss))


@pytest.mark.parametrize('tag', ['tiny_DAE_GRU', 'tiny_CNE_GRU_h48', 'full_DAE_GRU_g1p0'])
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


def _eval_model(tag):
    z, model = eval_fixture(tag)
    return z, model.cuda().train()


@pytest.mark.parametrize('cache', [False, True], ids=['per_sample', 'cached'])
def test_compute_scores_and_metrics_match_reference(cache):
    """A reference state_dict loads with strict=True; scores, ranks (the all-zero scores of a user without history included) and metrics."""
    from nnr_amd import evaluate as E
    z, model = _eval_model('tiny_DAE_GRU')
    assert float(np.abs(np.tanh(z['state/user_encoder.dec.bias'])).max()) > 1e-2 and bool((z['beh_history_mask'].sum(axis=1) == 0).any())
    dc = E.dev_corpus({k: z[k] for k in z.files}, 'cuda', int(z['category_num']))
    assert E.news_reps_cacheable(model) == bool(getattr(model.news_encoder, 'batch_independent', False))      # follows the news encoder, as for ATT
    scores = E.compute_scores(model, dc, batch_size=8, cache=cache and E.news_reps_cacheable(model))
    assert model.training
    got = scores.cpu().numpy()
    err = float(np.abs(got - z['scores']).max())
    print('eval_tiny_DAE_GRU scores max-abs-err %.3e (%s)' % (err, E.LAST_STATS['mode']))
    assert err <= 2e-5, err
    assert np.array_equal(got == 0.0, z['scores'] == 0.0) and bool((z['scores'] == 0.0).any())
    ranks, per, mean = E.rank_metrics(scores, torch.from_numpy(z['labels']), z['sizes'])
    np.testing.assert_array_equal(ranks.cpu().numpy(), z['ranks'])
    np.testing.assert_allclose(mean.cpu().numpy(), z['metrics'], rtol=0, atol=1e-12)
