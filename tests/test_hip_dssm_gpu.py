"""The DSSM baseline on the GPU: the weighted-bag kernels and the cosine click head + loss of csrc/dssm.hip against the float64 restatement
tests/dssm_ref.py (pinned to the reference by tests/test_dssm_host.py), and the model, trainer and scoring of nnr_amd/dssm.py against the
fixtures of tools/make_dssm_goldens.py.

Bars.  Op tests: tests/test_hip_bow_gpu.py's rule -- the same formula is evaluated in fp32 by CPU torch and compared with the float64
restatement; the kernel's bar is 4 x that error (the factor covers another summation order), never below 1e-6 x the expected tensor's max
magnitude.  Every measured value is printed.  Model tests: that file's TIGHT / LOGIT_TOL and its gradient rule, unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

import dssm_ref
from dssm_ref import DssmCase, PARAMS, f64, sample
from hip_masks import flat_keep

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4
TIGHT = 2e-5


def _chunk():
    from nnr_amd import ops
    return ops.wbag_dims(8, 1, 1)[0]


def _bag_shapes():
    """(na, La, nb, Lb, E, V): the smallest case | chunk boundaries, E on the 2-wide path | E odd | the workload's row lengths at two rows |
    one word: a single run spanning every workgroup of the backward | one word's run longer than one 64-chunk window of the backward's
    fix walk (65 chunks of 64 occurrences and one more: _LONG_RUN) | E > 512, the widest backward instance, with a run across a chunk edge."""
    ch = _chunk()
    return [(1, 1, 1, 1, 1, 2), (3, ch - 1, 2, ch + 1, 6, 11), (2, ch, 5, 3, 7, 5), (2, 3200, 3, 200, 512, 997), (4, 2 * ch + 5, 4, 9, 512, 1),
            (4, 4096, 2, 9, 8, 1), (2, 129, 2, 3, 516, 3)]


_BWD_CHUNK = 64                     # sorted occurrences per wave of the backward (csrc/dssm.hip: WB_BCH)
_LONG_RUN = 65 * _BWD_CHUNK + 1


def _live_words(c):
    """Word ids of the case's live occurrences (non-zero weight, id inside the table) in ascending order: the backward's sorted list
    without its pad entries."""
    V = c['shape'][5]
    words = []
    for ids, w, _, rows in (c['a'], c['b']):
        i, ww = ids[rows], w[rows]
        words.append(i[(ww != 0) & (i >= 0) & (i < V)].reshape(-1))
    return torch.cat(words).sort().values


def _bar(exp, fp32, name, report):
    """4 x the error of the same formula in fp32 on the CPU, floor 1e-6 x max |expected|."""
    e32, emax = float((fp32.double() - exp).abs().max()), float(exp.abs().max())
    bar = max(4.0 * e32, 1e-6 * emax)
    report.append('%s: fp32 formula %.3e, max|exp| %.3e, bar %.3e' % (name, e32, emax, bar))
    return bar


def _stream(g, n, L, V, with_sel, special):
    """One stream's term-vector table (ids, w), its selector and the rows the bag sees.  Weights are positive with zero tails of random
    length plus zero holes.  special (n > 1): table row 0, which the bag sees, has all-zero weights; the second row the bag sees is live
    at every position, carries ids -1 and V (when L > 1) and an id repeated inside the row (when L > 2).  The selector permutes the table
    (two of its rows are never selected) and, with more than two rows, names one row twice."""
    R = n + 2 if with_sel else n
    ids = torch.randint(0, V, (R, L), generator=g, dtype=torch.int32)
    w = torch.rand(R, L, generator=g) + 0.05
    tail = torch.randint(0, L + 1, (R,), generator=g)
    w[torch.arange(L)[None, :] >= (L - tail)[:, None]] = 0.0
    w[torch.rand(R, L, generator=g) < 0.1] = 0.0
    sel = None
    if with_sel:
        perm = torch.randperm(R, generator=g)
        if special:                                               # table row 0 first, then other rows in random order; with n > 2 one of them twice
            perm = torch.cat([torch.zeros(1, dtype=perm.dtype), perm[perm != 0]])
        sel = perm[:n].to(torch.int32)
        if special and n > 2:
            sel[-1] = sel[1]
    rows = sel.long() if sel is not None else torch.arange(n)
    if special:
        first = int(rows[1])                                      # a selected row other than table row 0
        w[first] = torch.rand(L, generator=g) + 0.05
        if L > 1:
            ids[first, 0], ids[first, L - 1] = -1, V
        if L > 2:
            ids[first, 2] = ids[first, 1]
        w[0] = 0.0                                                # a row of all-zero weights
    return ids, w, sel, rows


def _bag_case(shape, with_sel, p, seed):
    na, La, nb, Lb, E, V = shape
    g = torch.Generator().manual_seed(seed)
    special = na > 1 and nb > 1
    a = _stream(g, na, La, V, with_sel, special)
    b = _stream(g, nb, Lb, V, with_sel, special)
    table = torch.randn(V, E, generator=g)
    dout = torch.randn(na + nb, E, generator=g)
    prefill = 0.1 * torch.randn(V, E, generator=g)
    seeds = (1000 + seed, 2000 + seed)
    keeps = None
    if p > 0:      # the documented index: ((r * L + j) * E + e), r and j inside the stream
        keeps = (flat_keep(na * La * E, p, seeds[0]).view(na, La, E).cpu(), flat_keep(nb * Lb * E, p, seeds[1]).view(nb, Lb, E).cpu())
    return dict(shape=shape, a=a, b=b, table=table, dout=dout, prefill=prefill, seeds=seeds, keeps=keeps, p=p)


def _bag_expected(c, dtype):
    t = c['table'].to(dtype).clone().requires_grad_()
    outs = []
    for s, (ids, w, _, rows) in enumerate((c['a'], c['b'])):
        outs.append(dssm_ref.bag(t, ids[rows], w[rows].to(dtype), c['keeps'][s] if c['keeps'] else None, c['p']))
    out = torch.cat(outs, dim=0)
    (out * c['dout'].to(dtype)).sum().backward()
    return out.detach(), c['prefill'].to(dtype) + t.grad


def _bag_run(c, runs=2):
    from nnr_amd import ops
    na, La, nb, Lb, E, V = c['shape']
    dev = torch.device('cuda')

    def up(s):
        ids, w, sel, _ = s
        return ids.cuda().contiguous(), w.cuda().contiguous(), (sel.cuda().contiguous() if sel is not None else None)
    sa, sb = up(c['a']), up(c['b'])
    table, dout = c['table'].cuda(), c['dout'].cuda()
    outs, tables, plan = [], [], None
    for _ in range(runs):
        out = torch.full((na + nb, E), 7.0, device=dev)
        plan = ops.WbagPlan(na * La + nb * Lb, E, V, dev)
        ops.wbag_fwd(table, sa, sb, c['p'], c['seeds'][0], c['seeds'][1], out, plan)
        plan.sort()
        dt = c['prefill'].cuda().clone()
        ops.wbag_bwd(dout, sa, sb, c['p'], c['seeds'][0], c['seeds'][1], plan, dt)
        outs.append(out)
        tables.append(dt)
    torch.cuda.synchronize()
    return outs, tables, plan.tok


@pytest.mark.parametrize('p', [0.0, 0.5], ids=['p0', 'p0.5'])
@pytest.mark.parametrize('with_sel', [False, True], ids=['rows', 'sel'])
@pytest.mark.parametrize('index', range(7))
def test_weighted_bag_kernels_match_the_float64_restatement(index, with_sel, p):
    shape = _bag_shapes()[index]
    cases = [_bag_case(shape, with_sel, p, seed=17 + 5 * index + 2 * with_sel + (p > 0))]
    if shape[0] == 1:                                  # the row patterns one row cannot hold: a second call at four rows per stream
        cases.append(_bag_case((4, 3, 4, 3) + shape[4:], with_sel, p, seed=91 + with_sel + 2 * (p > 0)))
    # what the last two shapes are there for, checked on the CPU before anything runs
    words = _live_words(cases[0])
    if index == 5:
        assert int((words == 0).sum()) >= _LONG_RUN, int((words == 0).sum())
    if index == 6:
        edges = torch.arange(_BWD_CHUNK, words.numel(), _BWD_CHUNK)
        assert shape[4] > 512 and bool((words[edges] == words[edges - 1]).any()), words.numel()
    for c in cases:
        report = []
        exp_out, exp_dt = _bag_expected(c, f64)
        f32_out, f32_dt = _bag_expected(c, torch.float32)
        outs, tables, tok = _bag_run(c)
        bars = dict(out=_bar(exp_out, f32_out, 'out', report), dtable=_bar(exp_dt, f32_dt, 'dtable', report))
        errs = dict(out=float((outs[0].cpu().double() - exp_out).abs().max()), dtable=float((tables[0].cpu().double() - exp_dt).abs().max()))
        report.append('kernel: out %.3e, dtable %.3e' % (errs['out'], errs['dtable']))
        print('%s sel=%s p=%s: %s' % (c['shape'], with_sel, p, '; '.join(report)))
        assert errs['out'] <= bars['out'] and errs['dtable'] <= bars['dtable'], (c['shape'], errs, bars)
        assert torch.equal(outs[0], outs[1]) and torch.equal(tables[0], tables[1])          # same inputs, same bits
        # occurrence keys: the word id at live positions (non-zero weight, id inside the table), -1 elsewhere; stream a, then stream b
        V = c['shape'][5]
        toks, used = [], torch.zeros(V, dtype=torch.bool)
        for ids, w, _, rows in (c['a'], c['b']):
            i, ww = ids[rows], w[rows]
            live = (ww != 0) & (i >= 0) & (i < V)
            toks.append(torch.where(live, i, torch.full_like(i, -1)).reshape(-1))
            used[i[live].long()] = True
        assert torch.equal(tok.cpu(), torch.cat(toks))
        assert torch.equal(tables[0].cpu()[~used], c['prefill'][~used])                     # rows no live occurrence names keep their bits
        if p > 0 and c['keeps'][0].numel() > 64:
            assert abs(float(torch.cat([k.reshape(-1) for k in c['keeps']]).float().mean()) - 0.5) < 0.2      # masks, not all-ones


def test_bag_sizes_beyond_the_rule_are_unsupported():
    from nnr_amd import _lib, ops
    L = _lib.lib()
    dev = torch.device('cuda')
    f = torch.zeros(4096, device=dev)
    i = torch.zeros(4096, device=dev, dtype=torch.int32)
    s = torch.cuda.current_stream().cuda_stream
    for E, La, Lb in [(1025, 1, 1), (8, 4097, 1), (8, 1, 4097)]:
        # (the entry points answer before any launch: the small buffers are never touched)
        rc = L.nnr_wbag_fwd(f.data_ptr(), 4, E, i.data_ptr(), f.data_ptr(), None, 1, 1, La, i.data_ptr(), f.data_ptr(), None, 1, 1, Lb, 0.0, 1, 2,
                            f.data_ptr(), None, f.data_ptr(), s)
        assert rc == _lib.NNR_ERR_UNSUPPORTED, (E, La, Lb, rc)
        rc = L.nnr_wbag_bwd(f.data_ptr(), i.data_ptr(), i.data_ptr(), La + Lb, f.data_ptr(), None, 1, 1, La, f.data_ptr(), None, 1, 1, Lb, 4, E, 0.0, 1, 2,
                            f.data_ptr(), f.data_ptr(), s)
        assert rc == _lib.NNR_ERR_UNSUPPORTED, (E, La, Lb, rc)
    with pytest.raises(_lib.NnrHipError, match='unsupported size'):
        ops.wbag_fwd(torch.zeros(4, 1028, device=dev), (i[:8].view(2, 4), f[:8].view(2, 4), None), None, 0.0, 1, 2, torch.zeros(2, 1028, device=dev))
    torch.cuda.synchronize()
    assert float(f.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ cosine click head + loss
def _cosine_expected(u, v, dtype):
    u, v = u.to(dtype).clone().requires_grad_(), v.to(dtype).clone().requires_grad_()
    logits = dssm_ref.cosine_logits(u, v)
    logits.retain_grad()
    loss = dssm_ref.nls(logits)
    loss.backward()
    return dict(logits=logits.detach(), loss=loss.detach().reshape(1), dlogits=logits.grad, duser=u.grad, dnews=v.grad)


def _cosine_run(u, v, grads=True):
    from nnr_amd import ops
    B, N, F = v.shape
    dev = dict(device='cuda', dtype=torch.float32)
    ud, vd = u.cuda().contiguous(), v.cuda().contiguous()
    logits = torch.full((B, N), 7.0, **dev)
    if not grads:
        ops.cosine_loss(ud, vd, B, N, F, logits)
        return dict(logits=logits)
    loss, dlogits, du, dv, ws = torch.full((1,), 7.0, **dev), torch.empty((B, N), **dev), torch.empty((B, F), **dev), torch.empty((B, N, F), **dev), torch.empty(B, **dev)
    ops.cosine_loss(ud, vd, B, N, F, logits, loss, dlogits, du, dv, ws)
    return dict(logits=logits, loss=loss, dlogits=dlogits, duser=du, dnews=dv)


@pytest.mark.parametrize('shape', [(1, 1, 1), (2, 5, 3), (3, 64, 512), (7, 2, 130)], ids=lambda s: 'x'.join(str(v) for v in s))
def test_cosine_loss_matches_the_float64_restatement(shape):
    B, N, F = shape
    g = torch.Generator().manual_seed(B * 100 + N * 10 + F)
    u, v = torch.randn(B, F, generator=g), torch.randn(B, N, F, generator=g)
    exp, f32 = _cosine_expected(u, v, f64), _cosine_expected(u, v, torch.float32)
    got = _cosine_run(u, v)
    again = _cosine_run(u, v)
    evalc = _cosine_run(u, v, grads=False)
    torch.cuda.synchronize()
    report = []
    for k in ('logits', 'loss', 'dlogits', 'duser', 'dnews'):
        bar = _bar(exp[k], f32[k], k, report)
        err = float((got[k].cpu().double() - exp[k]).abs().max())
        report.append('kernel %s %.3e' % (k, err))
        assert err <= bar, (shape, k, err, bar, report)
        assert torch.equal(got[k], again[k])                                             # same inputs, same bits
    print('%s: %s' % (shape, '; '.join(report)))
    assert torch.equal(evalc['logits'], got['logits'])                                   # the eval call: the same logits bits


def test_cosine_loss_edges():
    from nnr_amd import _lib
    g = torch.Generator().manual_seed(5)
    u, v = torch.randn(2, 3, generator=g), torch.randn(2, 65, 3, generator=g)
    with pytest.raises(_lib.NnrHipError, match='unsupported size'):
        _cosine_run(u, v, grads=False)                                                   # N = 65
    u, v = torch.randn(3, 6, generator=g), torch.randn(3, 4, 6, generator=g)
    u[1] = 0.0
    logits = _cosine_run(u, v, grads=False)['logits'].cpu()
    assert bool(torch.isnan(logits[1]).all()) and bool(torch.isfinite(logits[[0, 2]]).all())      # the reference's 0 / 0, in that row only


# ------------------------------------------------------------------------------------------------ model, trainer, scoring
def _model(case, **over):
    from nnr_amd.dssm import DSSM
    model = DSSM(case.config(**over))
    model.load_state_dict({k: torch.as_tensor(v) for k, v in case.params().items()}, strict=True)
    return model.cuda()


def _corpus(case, **kw):
    from nnr_amd.dssm import DssmCorpus
    return DssmCorpus(case.expect('corpus/user_ids'), case.expect('corpus/user_w'), case.expect('corpus/news_ids'), case.expect('corpus/news_w'), 'cuda', **kw)


def _check_grads(model, exp_grads, total, report):
    """tests/test_hip_bow_gpu.py's rule: |d| <= 5e-5 x max(1e-3, the gradient's norm, 0.05 x the total norm)."""
    for k, p in model.named_parameters():
        exp = np.asarray(exp_grads[k], dtype=np.float64)
        got = sample(p.grad.detach().cpu().numpy()).astype(np.float64)
        norm = float(np.linalg.norm(exp)) * (p.numel() / exp.size) ** 0.5                 # (a sampled gradient: the norm of the whole, estimated)
        scale = max(1e-3, norm, 0.05 * total)
        err = float(np.abs(got - exp).max())
        report.append('d%s %.3e (bar %.3e)' % (k, err, 5e-5 * scale))
        assert err <= 5e-5 * scale, (k, err, scale)


@pytest.mark.parametrize('tag', ['dssm_tiny', 'dssm_tiny_wide'])
def test_model_matches_the_reference_fixture(tag):
    from nnr_amd.dssm import DssmTrainer
    case = DssmCase(tag)
    model = _model(case)
    model.train()
    batch = [torch.as_tensor(v).cuda() for v in case.batch()]
    trainer = DssmTrainer(model, case.config())
    logits, loss = trainer.forward_backward(batch)
    torch.cuda.synchronize()
    report = ['logits %.3e' % float(np.abs(logits.cpu().numpy() - case.expect('logits')).max()), 'loss %.3e' % abs(float(loss) - float(case.expect('loss')))]
    assert float(np.abs(logits.cpu().numpy() - case.expect('logits')).max()) <= LOGIT_TOL
    assert abs(float(loss) - float(case.expect('loss'))) <= TIGHT
    _check_grads(model, {k: case.expect('grad/' + k) for k in PARAMS}, float(case.expect('grad_total_norm')), report)
    assert abs(trainer.grad_total_norm() - float(case.expect('grad_total_norm'))) <= 2e-5 * max(1.0, float(case.expect('grad_total_norm')))
    with torch.no_grad():
        assert float((model(*batch) - logits).abs().max()) <= 1e-6                       # forward(): the same logits (dropout off at p = 0)
    lg2, loss2 = model.loss(*batch)                                                      # the autograd form of the loss
    assert torch.equal(lg2, logits) and torch.equal(loss2.detach(), loss)
    print('%s: %s' % (tag, '; '.join(report)))


def test_dropout_sites_through_the_restatement_fed_the_kernels_masks():
    """p = 0.5, training mode: the restatement gets the keep-masks the kernels will draw for the NEXT call (site seeds and index formulas as
    nnr_amd/dssm.py documents them), so logits, loss and every gradient compare element for element.  With five features a whole row of y
    is dropped now and then (0 / 0 in both implementations): the first model seed whose y masks keep a feature in every row is used."""
    from nnr_amd.dssm import DssmTrainer
    case = DssmCase('dssm_drop_tiny')
    ui, uw, _, ni, nw, _ = case.batch()
    B, N, Ln = ni.shape
    Lu, H, Fd, p = ui.shape[1], case.meta['DSSM_hidden_dim'], case.meta['DSSM_feature_dim'], case.p
    for model_seed in range(50):
        model = _model(case, seed=model_seed)
        seed = (model._seed_base + 7919 * (model._calls + 1)) & 0x7FFFFFFF
        l3 = flat_keep((B + B * N) * H, p, seed + 3).view(B + B * N, H).cpu()
        y = flat_keep((B + B * N) * Fd, p, seed + 4).view(B + B * N, Fd).cpu()
        if bool(y.any(dim=1).all()):
            break
    masks = dict(user_bag=flat_keep(B * Lu * H, p, seed + 1).view(B, Lu, H).cpu(), news_bag=flat_keep(B * N * Ln * H, p, seed + 2).view(B, N, Ln, H).cpu(),
                 user_l3=l3[:B], news_l3=l3[B:].view(B, N, H), user_y=y[:B], news_y=y[B:].view(B, N, Fd))
    rates = {k: float(v.float().mean()) for k, v in masks.items()}
    assert abs(np.mean([rates['user_bag'], rates['news_bag']]) - 0.5) < 0.15, rates
    exp_logits, exp_loss, exp_grads = dssm_ref.forward_backward(case.params(), ui, uw, ni, nw, masks, p)
    model.train()
    trainer = DssmTrainer(model, case.config())
    logits, loss = trainer.forward_backward([torch.as_tensor(v).cuda() for v in case.batch()])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(exp_loss))
    report = ['seed %d' % model_seed, 'logits %.3e' % float((logits.cpu().double() - exp_logits).abs().max()), 'loss %.3e' % abs(float(loss) - float(exp_loss))]
    assert float((logits.cpu().double() - exp_logits).abs().max()) <= LOGIT_TOL
    assert abs(float(loss) - float(exp_loss)) <= TIGHT
    total = float(torch.sqrt(sum((v ** 2).sum() for v in exp_grads.values())))
    _check_grads(model, {k: v.numpy() for k, v in exp_grads.items()}, total, report)
    print('; '.join(report))
    # eval mode: no dropout, whatever p says
    model.eval()
    ev = model(*[torch.as_tensor(v).cuda() for v in case.batch()])
    ref = dssm_ref.forward(dssm_ref.state(case.params()), *[torch.as_tensor(v) for v in (ui, uw, ni, nw)])[0]
    assert float((ev.cpu().double() - ref.detach()).abs().max()) <= LOGIT_TOL


@pytest.mark.parametrize('tag', ['dssm_tiny', 'dssm_tiny_wide'])
def test_forward_ids_equals_forward_on_the_gathered_tensors(tag):
    case = DssmCase(tag)
    model = _model(case).eval()
    corpus = _corpus(case)
    us, ns = torch.as_tensor(case.expect('in/user_sel')).cuda(), torch.as_tensor(case.expect('in/news_sel')).cuda()
    by_ids = model.forward_ids(corpus, us, ns)
    gathered = corpus.gather(us, ns)
    assert np.array_equal(gathered[0].cpu().numpy(), case.expect('in/user_indices')) and np.array_equal(gathered[4].cpu().numpy(), case.expect('in/news_weights'))
    by_tensors = model(*gathered)
    torch.cuda.synchronize()
    assert torch.equal(by_ids, by_tensors)                                               # bit for bit
    assert float(np.abs(by_ids.cpu().numpy() - case.expect('logits')).max()) <= LOGIT_TOL


@pytest.mark.parametrize('tag', ['dssm_tiny', 'dssm_tiny_wide'])
def test_trainer_reproduces_the_reference_steps(tag):
    from nnr_amd.dssm import DssmTrainer
    case = DssmCase(tag)
    steps, lr = int(case.meta['adam_steps']), float(case.meta['lr'])
    finals = []
    for run in range(2):
        model = _model(case)
        model.train()
        trainer = DssmTrainer(model, case.config())
        batch = [torch.as_tensor(v).cuda() for v in case.batch()] if run == 0 else (_corpus(case), torch.as_tensor(case.expect('in/user_sel')).cuda(),
                                                                                 torch.as_tensor(case.expect('in/news_sel')).cuda())
        for s in range(steps):
            _, loss = trainer.train_step(batch)
            err = abs(float(loss) - float(case.expect('loss_step%d' % s)))
            print('%s run %d step %d: loss error %.3e' % (tag, run, s, err))
            assert err <= 5e-5, (tag, s, err)
        torch.cuda.synchronize()
        for k, p in model.named_parameters():
            dlt = np.abs(sample(p.detach().cpu().numpy()) - case.expect('param%d/%s' % (steps, k)))
            assert dlt.max(initial=0.0) <= steps * lr * 1.01 + 1e-4, 'param (hard bound) ' + k
        finals.append(trainer.flat.flat.clone())
    assert torch.equal(finals[0], finals[1])                # two trainers from the same state (tensor batch / id-only batch): identical bits


@pytest.mark.parametrize('tag', ['dssm_tiny', 'dssm_tiny_wide', 'dssm_drop_tiny'])
def test_compute_scores_cached_and_per_sample(tag):
    from nnr_amd import dssm, evaluate
    case = DssmCase(tag)
    model = _model(case)
    su, sn = case.expect('eval/sample_user'), case.expect('eval/sample_news')
    corpus = _corpus(case, samples=(su, sn))
    cached = dssm.compute_scores(model, corpus, batch_size=5)
    per_sample = dssm.compute_scores(model, corpus, batch_size=5, cache=False)
    torch.cuda.synchronize()
    assert model.training                                                               # the mode is restored
    ui, uw = case.expect('corpus/user_ids')[su], case.expect('corpus/user_w')[su]
    ni, nw = case.expect('corpus/news_ids')[sn][:, None], case.expect('corpus/news_w')[sn][:, None]
    args = [torch.as_tensor(v) for v in (ui, uw, ni, nw)]
    exp = dssm_ref.forward(dssm_ref.state(case.params(), f64), *args)[0].detach().reshape(-1)
    f32 = dssm_ref.forward(dssm_ref.state(case.params(), torch.float32), *args)[0].detach().reshape(-1)
    report = []
    bar = _bar(exp, f32, 'scores', report)
    errs = (float((cached.cpu().double() - exp).abs().max()), float((per_sample.cpu().double() - exp).abs().max()),
            float((cached - per_sample).abs().max()))
    print('%s: %s; cached %.3e, per-sample %.3e, cached vs per-sample %.3e; reference fp32 %.3e' % (
        tag, report[0], errs[0], errs[1], errs[2], float(np.abs(case.expect('eval/scores').astype(np.float64) - exp.numpy()).max())))
    assert errs[0] <= bar and errs[1] <= bar and errs[2] <= 2 * bar, (errs, bar)
    labels, sizes = torch.as_tensor(case.expect('eval/labels')), case.expect('eval/sizes')
    for scores in (cached, per_sample):
        _, _, means = evaluate.rank_metrics(scores, labels, sizes)
        np.testing.assert_allclose(means.cpu().numpy(), case.expect('eval/metrics'), rtol=0, atol=1e-12)
