"""The news-encoder ablations CNE_Title / CNE_Content / CNE_wo_CS / CNE_wo_CA on the GPU: each encoder at the smallest shapes against the
float64 restatement (tests/cne_ablation_ref.py, pinned to the reference by tests/test_cne_ablation_host.py) through all three entry points,
with dropout off and on (the kernels' own keep-masks handed to the restatement); the model, state_dict and evaluation paths against golden
vectors captured from the reference's own code; bit reproducibility; and the data-parallel table-scatter hook count.  Bars as in
tests/test_hip_sue_ablation_gpu.py."""
import functools

import numpy as np
import pytest
import torch

import cne_ablation_ref as R
from golden_io import GoldenCase, build_model, eval_fixture

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4
TIGHT = 2e-5            # outputs, absolute
GRAD = 5e-5             # each gradient, of its own largest magnitude
NAMES = ['CNE_Title', 'CNE_Content', 'CNE_wo_CS', 'CNE_wo_CA']
CASES = ['tiny_CNE_Title_ATT', 'tiny_CNE_Content_ATT', 'tiny_CNE_wo_CS_ATT', 'tiny_CNE_wo_CS_SUE_stable', 'tiny_CNE_wo_CA_ATT_stable',
         'tiny_CNE_wo_CA_SUE_stable', 'full_CNE_Title_ATT_g1p0', 'full_CNE_wo_CS_ATT_g1p0', 'full_CNE_wo_CA_ATT_g1p0_stable']
LT, LC, E, A, V = 5, 9, 8, 4, 40
# lengths per call ((B, N) = (2, 3) candidates, (2, 4) history slots): an empty title / content (all-zero mask), full ones, ties
TITLE_LENS = {'news': [0, 5, 3, 3, 1, 2], 'user': [0, 5, 2, 2, 4, 4, 1, 3]}
CONTENT_LENS = {'news': [0, 9, 1, 4, 4, 7], 'user': [1, 9, 0, 3, 3, 6, 6, 2]}


def _cfg(name, H, p, seed=3):
    from nnr_amd import config
    return config.make_config([], news_encoder=name, user_encoder='ATT', vocabulary_size=V, word_embedding_dim=E, hidden_dim=H, attention_dim=A,
                              max_title_length=LT, max_abstract_length=LC, category_num=3, subCategory_num=7, dropout_rate=p, seed=seed,
                              tie_order='stable')


@functools.lru_cache(maxsize=None)
def _inputs():
    """The two calls' tensors on the CPU ({field: tensor}, Model.forward's names) and the upstream gradients' seeds."""
    g = torch.Generator().manual_seed(11)
    out = {}
    for call, (B, N) in (('news', (2, 3)), ('user', (2, 4))):
        for s, L, lens in (('title', LT, TITLE_LENS[call]), ('content', LC, CONTENT_LENS[call])):
            mask = torch.arange(L).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)
            text = torch.randint(1, V, (B * N, L), generator=g)
            text = torch.where(mask, text, torch.zeros_like(text))
            text[:, 0] = torch.where(mask[:, 0], text[:, 0], torch.randint(1, V, (B * N,), generator=g))      # an empty mask still reads a word
            out['%s_%s_text' % (call, s)], out['%s_%s_mask' % (call, s)] = text.view(B, N, L), mask.view(B, N, L)
        out[call + '_category'] = torch.randint(0, 3, (B, N), generator=g)
        out[call + '_subCategory'] = torch.randint(0, 7, (B, N), generator=g)
    return out


def _encoder_cpu(name, H, p):
    """The encoder on the CPU with weights that keep the comparison well conditioned.  initialize() is not used for the matrices: with
    E = 8 its orthogonal [4H, E] LSTM matrices give gate pre-activations of 0.1 |x|, the Bi-LSTM rows stay near zero, tanh(affine1) is
    the same for every token and -- the softmax being blind to a shift common to a sequence's scores -- affine1.bias' gradient cancels
    to 1e-3 of its terms, where fp32 rounding of the terms alone exceeds 5e-5 of the result.  Matrices are N(0, 4 / fan_in) instead
    (pre-activations and attention scores of O(1), rows that differ from token to token), biases N(0, 0.01), word rows N(0, 0.25)."""
    from nnr_amd import news_encoders
    cfg = _cfg(name, H, p)
    torch.manual_seed(7 + H)
    enc = getattr(news_encoders, name)(cfg, 0.5 * torch.randn(V, E))
    enc.initialize()
    with torch.no_grad():
        for k, q in enc.named_parameters():
            if q.dim() == 1:
                q.copy_(0.1 * torch.randn(q.shape))
            elif 'embedding' not in k:
                q.copy_(torch.randn(q.shape) * (2.0 / q.shape[1] ** 0.5))
    return enc, cfg


def _encoder(name, H, p):
    enc, cfg = _encoder_cpu(name, H, p)
    return enc.cuda().train(), cfg


def _call_args(dev, call):
    return tuple(dev['%s_%s' % (call, k)] for k in ('title_text', 'title_mask', 'content_text', 'content_mask', 'category', 'subCategory'))


def _run(name, H, p, mode, hook=None):
    """One forward + backward of both calls through `mode`; returns (got, the restatement's result, the device inputs after the call)."""
    import hip_masks
    from types import SimpleNamespace
    from nnr_amd import news_encoders as NE
    enc, cfg = _encoder(name, H, p)
    if hook is not None:
        enc.__dict__['_table_scatter_hook'] = hook
    cpu = _inputs()
    dev = {k: v.clone().cuda() for k, v in cpu.items()}
    D = enc.news_embedding_dim
    g = torch.Generator().manual_seed(13)
    douts = [torch.randn(2, 3, D, generator=g), torch.randn(2, 4, D, generator=g)]
    union = mode == 'pair'
    keep = hip_masks.cne_masks(SimpleNamespace(news_encoder=enc), dev, union=union) if p > 0 else None
    state = {'news_encoder.' + k: v.detach().cpu().numpy() for k, v in enc.state_dict().items()}
    exp = R.encode_batch(name, state, cfg, {k: v.numpy() for k, v in cpu.items()}, keep=keep, p=p, douts=douts)
    old = NE._CNE_UNION
    try:
        NE._CNE_UNION = mode != 'pair_lockstep'
        if mode == 'forward':
            c, h = _call_args(dev, 'news'), _call_args(dev, 'user')
            reps = [enc(c[0], c[1], None, c[2], c[3], None, c[4], c[5], None), enc(h[0], h[1], None, h[2], h[3], None, h[4], h[5], None)]
        else:
            reps = list(enc.forward_pair(_call_args(dev, 'news'), _call_args(dev, 'user')))
        torch.autograd.backward(reps, [d.cuda() for d in douts])
        torch.cuda.synchronize()
    finally:
        NE._CNE_UNION = old
    got = {'cand_rep': reps[0].detach(), 'hist_rep': reps[1].detach()}
    for k, q in enc.named_parameters():
        assert q.grad is not None, k
        got['grad/' + k] = q.grad
    return got, exp, dev, enc


def _check(got, exp, tag):
    report, worst = [], {}
    for k, e in exp.items():
        a = got[k].detach().cpu().double()
        assert bool(torch.isfinite(a).all()), (tag, k)
        err, emax = float((a - e).abs().max()), float(e.abs().max())
        bar = GRAD * emax if k.startswith('grad/') else TIGHT
        report.append('%s err %.3e (max|exp| %.3e, bar %.3e)' % (k, err, emax, bar))
        worst[k] = (err, bar)
    print(tag + ': ' + '; '.join(report))
    for k, (err, bar) in worst.items():
        assert err <= bar, (tag, k, err, bar)


@pytest.mark.parametrize('mode', ['forward', 'pair', 'pair_lockstep'])
@pytest.mark.parametrize('p', [0.0, 0.2], ids=['dropout_off', 'dropout_on'])
@pytest.mark.parametrize('H', [6, 200], ids=['one_cu', 'cu_pair'])
@pytest.mark.parametrize('name', NAMES)
def test_encoder_matches_the_float64_restatement(name, H, p, mode):
    from nnr_amd import ops
    got, exp, dev, enc = _run(name, H, p, mode)
    assert sorted(got) == sorted(exp)
    _check(got, exp, '%s H=%d p=%g %s' % (name, H, p, mode))
    assert ops.lstm_sync_timeouts() == 0
    # the in-place mask write reaches the masks the variant reads and no other; the unread stream's tensors are bit-identical
    cpu = _inputs()
    reads = enc.cne_streams
    for call in ('news', 'user'):
        for s in ('title', 'content'):
            orig = cpu['%s_%s_mask' % (call, s)]
            fixed = orig.clone()
            fixed[..., 0] = True
            assert not torch.equal(fixed, orig)
            assert torch.equal(dev['%s_%s_mask' % (call, s)].cpu(), fixed if s in reads else orig), (call, s)
            assert torch.equal(dev['%s_%s_text' % (call, s)].cpu(), cpu['%s_%s_text' % (call, s)])


@pytest.mark.parametrize('name', ['CNE_Title', 'CNE_wo_CA'])
def test_two_runs_give_bit_identical_gradients(name):
    """The same batch and the same seeds twice, dropout on, through the packed pair entry: every gradient bit for bit (the package's claim
    for CNE: fixed-order reductions everywhere)."""
    a, _, _, _ = _run(name, 200, 0.2, 'pair')
    b, _, _, _ = _run(name, 200, 0.2, 'pair')
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('mode', ['pair', 'pair_lockstep'])
@pytest.mark.parametrize('name', ['CNE_Content', 'CNE_wo_CS'])
def test_table_scatter_hook_is_called_as_often_as_it_is_told(name, mode):
    """Data parallel: the table's gradient bucket leaves when the hook has been called `count` times -- streams x calls."""
    seen = []
    _, _, _, enc = _run(name, 6, 0.0, mode, hook=seen.append)
    want = len(enc.cne_streams) * (1 if mode == 'pair' else 2)
    assert seen == [want] * want, (seen, want)


# ------------------------------------------------------------------------------------------------ model level
@pytest.mark.parametrize('tag', CASES)
def test_model_matches_reference_golden(tag):
    """The body of tests/test_hip_sue_ablation_gpu.py::test_model_matches_reference_golden, bars unchanged, with all four mutated masks."""
    from nnr_amd.trainer import Trainer
    from nnr_amd.model import negative_log_softmax
    case = GoldenCase(tag)
    model, cfg = build_model(case)
    trainer = Trainer(model, cfg)
    steps = int(case.meta['adam_steps'])
    rec = {}
    ne = model.news_encoder
    assert type(ne).__name__ == cfg.news_encoder
    orig_pair = ne.forward_pair

    def recording_pair(c, h):
        a, b = orig_pair(c, h)
        rec['reps'] = [a.detach().cpu().numpy(), b.detach().cpu().numpy()]
        return a, b
    ne.forward_pair = recording_pair
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
            # in-place input mutation is part of the reference's observable behaviour: all four text masks
            for key, idx in (('news_title', 16), ('news_content', 19), ('user_title', 4), ('user_content', 7)):
                np.testing.assert_array_equal(batch[idx].cpu().numpy(), case.expect('mutated_%s_mask' % key), err_msg=key)
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
    # the trainer's own step takes the autograd path for these pairs and records no tape
    for _ in range(4):
        _, loss = trainer.train_step(case.batch('cuda'))
        assert trainer.last_path == 'autograd'
    assert not trainer.tapes and bool(torch.isfinite(loss))


@pytest.mark.parametrize('tag', CASES)
def test_state_dict_of_the_fixtures_names_loads_strictly(tag):
    case = GoldenCase(tag)
    model, _ = build_model(case)
    shapes = {k: tuple(p.shape) for k, p in model.named_parameters()}
    st = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in case.initial_state(shapes).items()}
    assert sorted(st) == sorted(case.param_names())
    # (a state_dict lists the shared news encoder under the user encoder too; the fixture's names are named_parameters(), which does not)
    st.update({'user_encoder.' + k: v for k, v in st.items() if k.startswith('news_encoder.')})
    model.load_state_dict(st, strict=True)
    for k, p in model.named_parameters():
        assert torch.equal(p.detach().cpu(), st[k]), k


@pytest.mark.parametrize('tag,cached', [('tiny_CNE_wo_CS_ATT', True), ('tiny_CNE_wo_CA_ATT_stable', False)])
def test_reference_state_dict_loads_strictly_and_scores_match(tag, cached):
    """eval_fixture loads the reference's own state_dict with strict=True; evaluate.compute_scores on the cached path (CNE_wo_CS: a
    representation depends on its own news only) and on the per-sample path (CNE_wo_CA: never cached), bar as tests/test_hip_eval_gpu.py."""
    from nnr_amd import evaluate as E
    z, model = eval_fixture(tag)
    model = model.cuda().train()
    dc = E.dev_corpus({k: z[k] for k in z.files}, 'cuda', int(z['category_num']))
    assert E.news_reps_cacheable(model) is cached
    auto = E.compute_scores(model, dc, batch_size=8)
    assert E.LAST_STATS['mode'] == ('cached' if cached else 'per-sample') and model.training
    runs = [('auto', auto)]
    if cached:
        runs.append(('per-sample', E.compute_scores(model, dc, batch_size=8, cache=False)))
        assert E.LAST_STATS['mode'] == 'per-sample'
    assert E.LAST_STATS['pad_slots_skipped'] == 0                         # no inference de-duplication for the ablations
    for name, got in runs:
        err = float(np.abs(got.cpu().numpy() - z['scores']).max())
        print('%s %s scores max-abs-err %.3e' % (tag, name, err))
        assert err <= 2e-5, (name, err)
    ranks, _, mean = E.rank_metrics(auto, torch.from_numpy(z['labels']), z['sizes'])
    np.testing.assert_array_equal(ranks.cpu().numpy(), z['ranks'])
    np.testing.assert_allclose(mean.cpu().numpy(), z['metrics'], rtol=0, atol=1e-12)
