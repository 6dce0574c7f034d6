"""CPU checks of the single-view NAML news encoders NAML_Title / NAML_Content: flags and dispatch, the reference's parameter names and
shapes, initialize(), the float64 restatement the GPU tests compare against (tests/naml_ref.py) pinned to the reference's own results
(tests/golden/*NAML*.npz), the relu margins of the tiny fixtures, the per-table-row form of the category views, and the new entry points."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from golden_io import GoldenCase
from nnr_amd.synth import BATCH_FIELDS
import naml_ref

TINY = ['tiny_NAML_Title_ATT', 'tiny_NAML_Content_ATT', 'tiny_NAML_Content_CATT']
FULL = ['full_NAML_Title_ATT_g1p0']
DROP = 'drop_tiny_NAML_Content_ATT'
ENTRY_POINTS = ('nnr_view_pool_fwd', 'nnr_view_pool_bwd', 'nnr_conv1d_image_fwd', 'nnr_conv1d_dz_pad', 'nnr_conv1d_image_bwd')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-3
SIZES = dict(vocabulary_size=50)


def _model(case):
    from nnr_amd.model import Model
    return Model(case.config, case.word_table())


def _state(case):
    return case.initial_state({k: tuple(p.shape) for k, p in _model(case).named_parameters()})


def _batch(case):
    return {k: case.expect('in/' + k) for k in BATCH_FIELDS}


def test_flags_and_dispatch():
    from nnr_amd import config, news_encoders as NE, step, evaluate
    from nnr_amd.model import Model
    assert config.ALL_NEWS_ENCODERS == config.NEWS_ENCODERS + ['NAML_Title', 'NAML_Content']
    for name, cls, stream, L in (('NAML_Title', NE.NAML_Title, 'title', 32), ('NAML_Content', NE.NAML_Content, 'content', 128)):
        for user in ('ATT', 'CATT'):
            m = Model(config.make_config(['--news_encoder=' + name, '--user_encoder=' + user], corpus_sizes=SIZES))
            ne = m.news_encoder
            assert type(ne) is cls and ne.batch_independent and ne.max_length == L
            assert m.news_embedding_dim == ne.news_embedding_dim == 400                     # cnn_kernel_num: no feature fusion
            assert step.kind(m) is None and evaluate.news_reps_cacheable(m) and not m.use_user_embedding and ne.auxiliary_loss is None
            conv = getattr(ne, stream + '_conv').conv
            assert tuple(conv.weight.shape) == (400, 300, 3) and conv.padding == (1,)
            assert tuple(ne.category_affine.weight.shape) == (400, 50) and tuple(ne.affine1.weight.shape) == (200, 400)
            assert tuple(ne.affine2.weight.shape) == (1, 200) and ne.affine2.bias is None
    m = Model(config.make_config(['--news_encoder=NAML_Content', '--user_encoder=ATT', '--cnn_kernel_num=30', '--cnn_window_size=5',
                                  '--max_abstract_length=17', '--attention_dim=12'], corpus_sizes=SIZES))
    ne = m.news_encoder
    assert m.news_embedding_dim == 30 and ne.max_content_length == 17 and tuple(ne.content_conv.conv.weight.shape) == (30, 300, 5)
    assert tuple(ne.content_attention.affine1.weight.shape) == (12, 30)


def test_refusals():
    from nnr_amd import config
    from nnr_amd.model import Model
    with pytest.raises(Exception, match='PNE, DAE, Inception, KCNN, NAML_Title, NAML_Content'):
        Model(config.make_config(['--news_encoder=NAML'], corpus_sizes=SIZES))
    for name in ('NAML_Title', 'NAML_Content'):
        for k in (2, 4):
            with pytest.raises(Exception, match='unsupported size'):
                Model(config.make_config(['--news_encoder=' + name, '--user_encoder=ATT', '--cnn_window_size=%d' % k], corpus_sizes=SIZES))
        with pytest.raises(AssertionError, match='only cnn_method=naive'):
            Model(config.make_config(['--news_encoder=' + name, '--user_encoder=ATT', '--cnn_method=group3'], corpus_sizes=SIZES))


def _reference_names(stream):
    """variantEncoders.py:104-113 on top of newsEncoders.py:11-24, in the reference's registration order."""
    return (['word_embedding.weight', 'category_embedding.weight', 'subCategory_embedding.weight', stream + '_conv.conv.weight', stream + '_conv.conv.bias'] +
            [stream + '_attention.' + k for k in ('affine1.weight', 'affine1.bias', 'affine2.weight')] +
            ['category_affine.weight', 'category_affine.bias', 'subCategory_affine.weight', 'subCategory_affine.bias', 'affine1.weight', 'affine1.bias',
             'affine2.weight'])


@pytest.mark.parametrize('name,stream', [('NAML_Title', 'title'), ('NAML_Content', 'content')])
def test_a_reference_shaped_state_dict_loads_strictly(name, stream):
    from nnr_amd import config
    from nnr_amd.model import Model
    m = Model(config.make_config(['--news_encoder=' + name, '--user_encoder=ATT', '--cnn_kernel_num=12', '--attention_dim=8', '--word_embedding_dim=16'],
                                 corpus_sizes=SIZES))
    ne = m.news_encoder
    assert list(ne.state_dict().keys()) == _reference_names(stream)
    shapes = {'word_embedding.weight': (50, 16), 'category_embedding.weight': (18, 50), 'subCategory_embedding.weight': (285, 50),
              stream + '_conv.conv.weight': (12, 16, 3), stream + '_conv.conv.bias': (12,), stream + '_attention.affine1.weight': (8, 12),
              stream + '_attention.affine1.bias': (8,), stream + '_attention.affine2.weight': (1, 8), 'category_affine.weight': (12, 50),
              'category_affine.bias': (12,), 'subCategory_affine.weight': (12, 50), 'subCategory_affine.bias': (12,), 'affine1.weight': (8, 12),
              'affine1.bias': (8,), 'affine2.weight': (1, 8)}
    g = torch.Generator().manual_seed(3)
    sd = {k: torch.randn(shapes[k], generator=g) for k in _reference_names(stream)}
    res = ne.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in sd.items():
        assert torch.equal(ne.state_dict()[k], v), k


@pytest.mark.parametrize('name,stream', [('NAML_Title', 'title'), ('NAML_Content', 'content')])
def test_initialize_draws_the_reference_distributions(name, stream):
    """variantEncoders.py:115-124: xavier_uniform_ with gain 1 for the two category affines and affine1 (NOT Attention's tanh gain), zero
    biases, xavier for affine2; the text attention initialises itself with the tanh gain; the convolution stays as torch made it."""
    from nnr_amd import config
    from nnr_amd.model import Model
    torch.manual_seed(0)
    m = Model(config.make_config(['--news_encoder=' + name, '--user_encoder=ATT'], corpus_sizes=SIZES))
    ne = m.news_encoder
    conv = getattr(ne, stream + '_conv').conv
    keep = (conv.weight.detach().clone(), conv.bias.detach().clone())
    with torch.no_grad():
        for lin in (ne.category_affine, ne.subCategory_affine, ne.affine1):
            lin.bias.fill_(1.0)
    m.initialize()
    assert torch.equal(conv.weight.detach(), keep[0]) and torch.equal(conv.bias.detach(), keep[1])
    for lin, gain in ((ne.category_affine, 1.0), (ne.subCategory_affine, 1.0), (ne.affine1, 1.0), (ne.affine2, 1.0),
                      (getattr(ne, stream + '_attention').affine1, 5.0 / 3.0), (getattr(ne, stream + '_attention').affine2, 1.0)):
        fan_out, fan_in = lin.weight.shape
        bound = gain * math.sqrt(6.0 / (fan_in + fan_out))
        top = float(lin.weight.detach().abs().max())
        assert 0.9 * bound < top <= bound * (1 + 1e-6), (tuple(lin.weight.shape), top, bound)
        if lin.bias is not None:
            assert float(lin.bias.detach().abs().max()) == 0.0
    assert float(ne.subCategory_embedding.weight[0].abs().max()) == 0.0 and float(ne.category_embedding.weight.abs().max()) <= 0.1


@pytest.mark.parametrize('tag', TINY + FULL + [DROP])
def test_model_constructs_with_the_reference_parameters(tag):
    case = GoldenCase(tag)
    model = _model(case)
    case.load_into(model)                                    # names equal the reference's named_parameters()
    if case.full_arrays:
        for k, p in model.named_parameters():
            assert tuple(p.shape) == tuple(case.expect('param1/' + k).shape), k
    assert model.news_embedding_dim == int(case.config.cnn_kernel_num)
    biases = [k for k, p in _state(case).items() if k.startswith('news_encoder.') and k.endswith('.bias')]
    assert len(biases) == 5 and all(float(np.abs(_state(case)[k]).max()) > 0 for k in biases)      # random biases: the bias paths count


@pytest.mark.parametrize('tag', TINY)
def test_the_fixtures_decide_every_relu(tag):
    """In the reference's float64 run no relu pre-activation -- the convolution outputs and both category affines of both encoder calls --
    lies within 1e-3 of its tensor's scale of zero, and the restatement's pre-activations are the reference's.  So no fp32 sign flip can
    excuse a mismatch, and the GPU tests exempt no element."""
    case = GoldenCase(tag)
    out = naml_ref.model_forward(case.config, _state(case), _batch(case))
    for call in ('cand', 'hist'):
        for k in ('z', 'za', 'zs'):
            ref = torch.from_numpy(case.expect('f64/naml/%s_%s' % (k, call)))
            mine = out['pre'][call][k].detach().reshape(ref.shape)
            assert float((mine - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), (call, k)
            ratio = float(ref.abs().min() / ref.abs().max())
            print('%s %s %s: smallest |pre-activation| %.2e of the scale' % (tag, call, k, ratio))
            assert ratio >= MARGIN, (tag, call, k, ratio)
            assert bool((ref > 0).any()) and bool((ref < 0).any()), (call, k)                 # both sides of the relu occur


def _rel(got, exp):
    exp = naml_ref.f64(exp)
    return float((got.detach().reshape(exp.shape) - exp).abs().max()), float(exp.abs().max())


@pytest.mark.parametrize('tag', TINY)
def test_restatement_reproduces_the_reference(tag):
    """cand_rep, hist_rep, logits, loss and every stored gradient: to 1e-9 of each tensor's own scale against the reference's float64 run
    stored in the fixture (float64 against float64; a floor of 1e-12 for gradients that are zero on paper), and to 2e-5 of the scale against
    its fp32 results (which carry the reference's own fp32 rounding)."""
    case = GoldenCase(tag)
    out = naml_ref.model_forward(case.config, _state(case), _batch(case))
    out['loss'].backward()
    items = [('cand_rep', out['cand_rep']), ('hist_rep', out['hist_rep']), ('logits', out['logits']), ('loss', out['loss'])]
    items += [('grad/' + k, p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in out['state'].items()]
    report = []
    for name, got in items:
        e64, s64 = _rel(got, case.expect('f64/' + name))
        assert e64 <= max(1e-9 * s64, 1e-12), (tag, name, 'float64', e64, s64)
        e32, s32 = _rel(got, case.expect(name))
        report.append('%s f64 %.1e fp32 %.1e' % (name, e64 / max(s64, 1e-300), e32 / max(s32, 1e-300)))
        assert e32 <= 2e-5 * s32 + 1e-9, (tag, name, 'fp32', e32, s32)
    print(tag + ': ' + '; '.join(report))


def test_restatement_reproduces_the_reference_at_full_size():
    """The full-size fixture stores the fp32 run's logits and loss and 64-element slices of every gradient."""
    case = GoldenCase(FULL[0])
    out = naml_ref.model_forward(case.config, _state(case), _batch(case))
    out['loss'].backward()
    for name, got in (('logits', out['logits']), ('loss', out['loss'])):
        e, s = _rel(got, case.expect(name))
        assert e <= 2e-5 * s, (name, e, s)
    for k, p in out['state'].items():
        exp = case.expect('grad/' + k)
        got = p.grad.reshape(-1)[:64].numpy()
        gn = float(case.expect('gradnorm/' + k))
        assert abs(float(p.grad.norm()) - gn) <= 1e-4 * gn + 1e-9, k
        assert float(np.abs(got - exp).max()) <= 1e-4 * float(p.grad.abs().max()) + 1e-9, k


def test_restatement_with_the_recorded_masks_reproduces_the_dropout_run():
    """drop_tiny_NAML_Content_ATT: the reference in train mode at 0.25, its four masks in call order -- word rows then convolution output, of
    the candidate call then of the history call -- each applied as keep / (1 - p).  Pins the two sites' order, rate, shape and scale."""
    case = GoldenCase(DROP)
    calls = case.dropout_calls()
    cfg = case.config
    B, N, L = case.expect('in/news_content_text').shape
    H = case.expect('in/user_content_text').shape[1]
    E, C = int(cfg.word_embedding_dim), int(cfg.cnn_kernel_num)
    assert [p for p, _ in calls] == [0.25] * 4
    assert [tuple(k.shape) for _, k in calls] == [(B, N, L, E), (B * N, L, C), (B, H, L, E), (B * H, L, C)]
    keeps = (dict(word=calls[0][1].reshape(B * N, L, E), conv=calls[1][1]), dict(word=calls[2][1].reshape(B * H, L, E), conv=calls[3][1]))
    out = naml_ref.model_forward(cfg, _state(case), _batch(case), p=0.25, keeps=keeps)
    out['loss'].backward()
    for name, got in [('cand_rep', out['cand_rep']), ('hist_rep', out['hist_rep']), ('logits', out['logits']), ('loss', out['loss'])] + \
                     [('grad/' + k, p.grad) for k, p in out['state'].items()]:
        e, s = _rel(got, case.expect(name))
        assert e <= 2e-5 * s + 1e-9, (name, e, s)
    plain = naml_ref.model_forward(cfg, _state(case), _batch(case))
    assert float((plain['logits'] - out['logits']).abs().max()) > 1e-3                        # the masks matter


@pytest.mark.parametrize('tag', ['tiny_NAML_Title_ATT', 'tiny_NAML_Content_CATT'])
def test_per_table_row_form_equals_the_per_news_form(tag):
    """relu(affine(table))[id] with its score computed once per table row (what csrc/naml.hip indexes) against relu(affine(table[id])) per
    news, in float64: values and every gradient to 1e-12 of the scale."""
    case = GoldenCase(tag)
    a = naml_ref.model_forward(case.config, _state(case), _batch(case))
    b = naml_ref.model_forward(case.config, _state(case), _batch(case), per_row=True)
    a['loss'].backward()
    b['loss'].backward()
    for k in ('cand_rep', 'hist_rep', 'logits'):
        assert float((a[k] - b[k]).abs().max()) <= 1e-12 * float(a[k].abs().max()), k
    for k, p in a['state'].items():
        q = b['state'][k]
        s = float(p.grad.abs().max())
        assert float((p.grad - q.grad).abs().max()) <= 1e-12 * max(s, 1e-3), k


def test_view_pool_restatement_for_two_text_views():
    """naml_ref.view_pool at op level: Vt = 1 equals the stacked softmax of the encoder form; Vt = 2 adds a view between the text view and
    the table views; the weights sum to one and a score of -80 against +80 leaves its view a weight of exactly zero in float64."""
    g = torch.Generator().manual_seed(2)
    n, C, Ra, Rb = 5, 7, 3, 4
    t0, t1 = torch.randn(n, C, generator=g).double(), torch.randn(n, C, generator=g).double()
    rowsA, rowsB = torch.randn(Ra, C, generator=g).double(), torch.randn(Rb, C, generator=g).double()
    s0, s1 = torch.randn(n, generator=g).double(), torch.randn(n, generator=g).double()
    sa, sb = torch.randn(Ra, generator=g).double(), torch.randn(Rb, generator=g).double()
    ia, ib = torch.tensor([0, 2, 2, 0, 2]), torch.tensor([3, 3, 3, 3, 3])
    out1, al1 = naml_ref.view_pool([t0], [s0], rowsA, sa, ia, rowsB, sb, ib)
    F = torch.stack([t0, rowsA[ia], rowsB[ib]], dim=1)
    al = torch.softmax(torch.stack([s0, sa[ia], sb[ib]], dim=1), dim=1)
    assert torch.equal(out1, (F * al.unsqueeze(2)).sum(dim=1)) and tuple(al1.shape) == (n, 3)
    out2, al2 = naml_ref.view_pool([t0, t1], [s0, s1], rowsA, sa, ia, rowsB, sb, ib)
    assert tuple(al2.shape) == (n, 4) and float((al2.sum(dim=1) - 1).abs().max()) <= 1e-15
    s1[:] = -80.0
    s0[:] = 80.0
    out3, al3 = naml_ref.view_pool([t0, t1], [s0, s1], rowsA, sa, ia, rowsB, sb, ib)
    assert float(al3[:, 1].max()) < 1e-60 and float((out3 - t0).abs().max()) < 1e-30


def test_entry_points_are_declared_listed_and_exported():
    from nnr_amd import _lib, profile
    header = open(os.path.join(ROOT, 'include', 'nnr_hip.h')).read()
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert _lib.lib().nnr_tape_fn_id(name.encode()) >= 0, name
    assert profile.HBM_KERNELS_OTHER['view_pool_fwd'] == (('view_pool_fwd_kernel',), 1)
    assert profile.HBM_KERNELS_OTHER['view_pool_bwd'] == (('view_pool_bwd_news_kernel', 'view_pool_bwd_table_kernel'), 2)
    assert open(os.path.join(ROOT, 'nnr_amd', 'csrc', 'build.sh')).read().count(' naml ') == 1
    # the refusals need no device: sizes are checked before any pointer is touched
    L = _lib.lib()
    for n, C, Ra, Rb, Vt in ((0, 4, 3, 3, 1), (-1, 4, 3, 3, 1), (4, 0, 3, 3, 1), (4, 4, 0, 3, 1), (4, 4, 3, -2, 1), (4, 4, 3, 3, 0), (4, 4, 3, 3, 3)):
        assert L.nnr_view_pool_fwd(None, None, None, None, Vt, None, None, None, Ra, None, None, None, Rb, n, C, None, None, None) == _lib.NNR_ERR_UNSUPPORTED
        assert L.nnr_view_pool_bwd(None, None, None, Vt, None, None, Ra, None, None, Rb, None, n, C, None, None, None, None, None, None, None, None,
                                   None, None) == _lib.NNR_ERR_UNSUPPORTED
    assert L.nnr_view_pool_fwd(None, None, None, None, 1, None, None, None, 3, None, None, None, 3, 4, 4, None, None, None) not in (0, _lib.NNR_ERR_UNSUPPORTED)
    for n, Lx, E, k in ((0, 5, 8, 3), (2, 0, 8, 3), (2, 5, 0, 3), (2, 5, 8, 2), (2, 9, 8, 9), (2, 5, 8, -1)):
        assert L.nnr_conv1d_image_fwd(None, 3, None, n, Lx, E, k, 0.0, 0, None, None) == _lib.NNR_ERR_UNSUPPORTED
        assert L.nnr_conv1d_dz_pad(None, None, n, Lx, E, k, None, None) == _lib.NNR_ERR_UNSUPPORTED
        assert L.nnr_conv1d_image_bwd(None, n, Lx, E, k, 0.0, 0, None, None) == _lib.NNR_ERR_UNSUPPORTED
    assert profile.HBM_KERNELS_OTHER['conv1d_dz_pad'] == (('conv1d_dz_pad_kernel',), 1)
