"""CPU checks of the bag-of-words news encoders DAE and Inception: flags, constructor asserts, the reference's parameter names and shapes,
the float64 restatements the GPU tests compare against (tests/bow_ref.py) pinned to the reference's own results (tests/golden/*DAE*.npz,
*Inception*.npz), the history-call-wins behaviour of DAE's auxiliary loss, torch's zero-distance norm gradient, and the new entry points."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from golden_io import GoldenCase
from nnr_amd.synth import BATCH_FIELDS
import bow_ref

TINY = ['tiny_DAE_ATT', 'tiny_DAE_CATT', 'tiny_Inception_ATT', 'tiny_Inception_CATT']
FULL = ['full_DAE_ATT_g1p0', 'full_Inception_ATT_g1p0']
ENTRY_POINTS = ('nnr_bag_mean_fwd', 'nnr_bag_mean_bwd', 'nnr_bag_mean_bwd_ws_floats', 'nnr_row_dist_fwd', 'nnr_row_dist_bwd', 'nnr_sigmoid_drop_bwd')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(case):
    from nnr_amd.model import Model
    return Model(case.config, case.word_table())


def _state(case):
    return case.initial_state({k: tuple(p.shape) for k, p in _model(case).named_parameters()})


def _batch(case):
    return {k: case.expect('in/' + k) for k in BATCH_FIELDS}


def test_flags():
    from nnr_amd import config
    assert 'DAE' in config.NEWS_ENCODERS and 'Inception' in config.NEWS_ENCODERS
    assert config.NEWS_ENCODERS[:4] == ['CNE', 'CNN', 'MHSA', 'PNE']
    cfg = config.make_config([], corpus_sizes=dict(vocabulary_size=50))
    assert cfg.Alpha == 0.1 and isinstance(cfg.Alpha, float)
    assert config.make_config(['--Alpha=0.25'], corpus_sizes=dict(vocabulary_size=50)).Alpha == 0.25


def test_constructor_asserts_and_dispatch():
    from nnr_amd.config import make_config
    from nnr_amd.model import Model
    from nnr_amd import news_encoders as NE, step, evaluate
    sizes = dict(vocabulary_size=50)
    m = Model(make_config(['--news_encoder=DAE', '--user_encoder=ATT'], corpus_sizes=sizes))
    assert type(m.news_encoder) is NE.DAE and m.news_embedding_dim == 200 + 50 + 50 and step.kind(m) is None
    assert evaluate.news_reps_cacheable(m) and not m.use_user_embedding and m.news_encoder.auxiliary_loss is None
    with pytest.raises(AssertionError, match='Reconstruction loss weight must be greater than 0'):
        Model(make_config(['--news_encoder=DAE', '--user_encoder=ATT', '--Alpha=0'], corpus_sizes=sizes))
    with pytest.raises(AssertionError, match='embedding dimension must be the same in the Inception module'):
        Model(make_config(['--news_encoder=Inception', '--user_encoder=CATT'], corpus_sizes=sizes))                    # 300 / 50 / 50
    m = Model(make_config(['--news_encoder=Inception', '--user_encoder=CATT', '--category_embedding_dim=300', '--subCategory_embedding_dim=300'],
                          corpus_sizes=sizes))
    assert type(m.news_encoder) is NE.Inception and m.news_embedding_dim == 300 and step.kind(m) is None and evaluate.news_reps_cacheable(m)
    with pytest.raises(Exception, match='DAE, Inception'):
        Model(make_config(['--news_encoder=NAML'], corpus_sizes=sizes))


@pytest.mark.parametrize('tag', TINY + FULL)
def test_model_constructs_with_the_reference_parameters(tag):
    case = GoldenCase(tag)
    cfg = case.config
    model = _model(case)
    case.load_into(model)                                    # names equal the reference's named_parameters()
    sd = dict(model.named_parameters())
    if case.full_arrays:
        for k, p in sd.items():
            assert tuple(p.shape) == tuple(case.expect('param1/' + k).shape), k
    E, H = int(cfg.word_embedding_dim), int(cfg.hidden_dim)
    if cfg.news_encoder == 'DAE':
        assert tuple(sd['news_encoder.f1.weight'].shape) == (H, E) and tuple(sd['news_encoder.f2.weight'].shape) == (E, H)
        assert model.news_embedding_dim == H + int(cfg.category_embedding_dim) + int(cfg.subCategory_embedding_dim)
    else:
        shapes = {'fc1_1': (H, 4 * E), 'fc1_2': (H, H), 'fc1_3': (E, H), 'fc2': (E, 4 * E), 'linear_transform': (E, 3 * E)}
        for k, s in shapes.items():
            assert tuple(sd['news_encoder.%s.weight' % k].shape) == s and tuple(sd['news_encoder.%s.bias' % k].shape) == s[:1]
        assert model.news_embedding_dim == E
    model.initialize()
    for k, p in model.named_parameters():
        if k.startswith('news_encoder.f') and k.endswith('.bias'):
            assert float(p.detach().abs().max()) == 0.0, k


# Gradient tensors of the fixtures whose stored fp32 value is further than 1e-6 of the tensor's own max from the reference's OWN float64 run
# (`f64/grad/...` in the same fixture), with that measured distance: sums of cancelling terms, or a gradient that is zero on paper (CATT's
# affine2.bias; the candidate columns and the bias of an always-active affine1 unit).  Each is held to 1.5 x its measured value against fp32
# -- and, like every tensor, to 1e-6 against the float64 run, which is what pins the restatement.
FP32_EXCEPTIONS = {
    ('tiny_DAE_ATT', 'grad/news_encoder.category_embedding.weight'): 1.24e-6,
    ('tiny_DAE_ATT', 'grad/news_encoder.f1.bias'): 4.00e-6,
    ('tiny_DAE_ATT', 'grad/news_encoder.f1.weight'): 1.97e-6,
    ('tiny_DAE_ATT', 'grad/user_encoder.attention.affine1.bias'): 2.67e-6,
    ('tiny_DAE_CATT', 'grad/news_encoder.f1.bias'): 2.05e-6,
    ('tiny_DAE_CATT', 'grad/news_encoder.f1.weight'): 1.75e-6,
    ('tiny_DAE_CATT', 'grad/user_encoder.affine1.bias'): 1.76e-5,
    ('tiny_DAE_CATT', 'grad/user_encoder.affine1.weight'): 8.78e-6,
    ('tiny_DAE_CATT', 'grad/user_encoder.affine2.weight'): 2.38e-5,
    ('tiny_DAE_CATT', 'grad/user_encoder.affine2.bias'): 1.0,          # zero on paper: 5e-17 in float64, rounding noise of 1e-9 in fp32
    ('tiny_Inception_CATT', 'grad/user_encoder.affine1.bias'): 1.81e-6,
    ('tiny_Inception_CATT', 'grad/user_encoder.affine2.bias'): 1.0,    # zero on paper
}


def _rel(got, exp):
    exp = bow_ref.f64(exp)
    return float((got.detach().reshape(exp.shape) - exp).abs().max()), float(exp.abs().max())


@pytest.mark.parametrize('tag', TINY)
def test_restatement_reproduces_the_reference(tag):
    """cand_rep, hist_rep, auxiliary_loss, logits, loss and every stored gradient to 1e-6 of each tensor's own scale (max |expected|), twice:
    against the reference's float64 run stored in the fixture (every tensor, no exception; a floor of 1e-12, float64 rounding of O(1) sums,
    for gradients that are zero on paper), and against its fp32 results (every tensor but those named in FP32_EXCEPTIONS, whose fp32 value
    is itself further than that from the float64 run)."""
    case = GoldenCase(tag)
    out = bow_ref.model_forward(case.config, _state(case), _batch(case))
    out['loss'].backward()
    report, seen = [], set()
    items = [('cand_rep', out['cand_rep']), ('hist_rep', out['hist_rep']), ('logits', out['logits']), ('loss', out['loss'])]
    if case.config.news_encoder == 'DAE':
        items.append(('auxiliary_loss', out['aux']))
    else:
        assert 'auxiliary_loss' not in case.z.files
    items += [('grad/' + k, p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in out['state'].items()]
    for name, got in items:
        e64, s64 = _rel(got, case.expect('f64/' + name))
        assert e64 <= max(1e-6 * s64, 1e-12), (tag, name, 'float64', e64, s64)
        e32, s32 = _rel(got, case.expect(name))
        rel = e32 / s32 if s32 > 0 else (0.0 if e32 == 0 else float('inf'))
        report.append('%s f64 %.1e fp32 %.2e (max %.2e)' % (name, e64 / max(s64, 1e-300), rel, s32))
        if (tag, name) in FP32_EXCEPTIONS:
            seen.add((tag, name))
            assert 1e-6 < rel <= 1.5 * FP32_EXCEPTIONS[(tag, name)], (tag, name, rel)
        else:
            assert rel <= 1e-6, (tag, name, 'fp32', rel, s32)
    for k in out['state']:
        g = out['state'][k].grad
        gn = float(case.expect('gradnorm/' + k))
        assert abs((float(g.norm()) if g is not None else 0.0) - gn) <= 1e-6 * gn + 1e-12 or (tag, 'grad/' + k) in FP32_EXCEPTIONS, (tag, k)
    assert seen == {key for key in FP32_EXCEPTIONS if key[0] == tag}
    print(tag + ': ' + '; '.join(report))


@pytest.mark.parametrize('tag', [t for t in TINY if '_DAE_' in t])
def test_the_history_call_wins(tag):
    """DAE rewrites auxiliary_loss in every call: what the trainer adds is the HISTORY call's mean; the candidate call's is elsewhere."""
    case = GoldenCase(tag)
    out = bow_ref.model_forward(case.config, _state(case), _batch(case))
    stored = float(case.expect('auxiliary_loss'))
    assert abs(float(case.expect('dae/aux_hist')) - stored) <= 1e-7
    assert abs(float(out['aux']) - stored) <= 1e-6 * stored
    assert abs(float(out['aux_cand']) - float(case.expect('dae/aux_cand'))) <= 1e-6 * stored
    assert abs(float(out['aux_cand']) - stored) > 1e-3
    assert stored >= 0.01 * float(case.expect('loss'))


def test_torch_gives_a_zero_gradient_at_zero_distance():
    a = torch.tensor([[1.0, 2.0, 3.0], [0.5, -1.0, 2.0]], requires_grad=True)
    b = torch.tensor([[1.0, 2.0, 3.0], [0.0, 1.0, 2.0]], requires_grad=True)
    aux = torch.norm(a - b, dim=1, keepdim=False) * 0.1
    aux.mean().backward()
    assert float(aux[0]) == 0.0 and float(a.grad[0].abs().max()) == 0.0 and float(b.grad[0].abs().max()) == 0.0
    assert bool(torch.isfinite(a.grad).all()) and bool(torch.isfinite(b.grad).all()) and float(a.grad[1].abs().max()) > 0.0
    # the restatement's sqrt form has no such subgradient; the GPU test therefore takes the expected gradient of an a == b row from torch.norm
    d = bow_ref.row_dist(a.detach().double(), b.detach().double(), 0.1)
    assert float(d[0]) == 0.0 and abs(float(d[1]) - float(aux[1])) <= 1e-7


def test_bag_mean_modes():
    """joint = one mean over both streams; separate = one mean per stream with position 0 forced live; a live id 0 and a repeated id count."""
    table = torch.arange(12.0, dtype=torch.float64).reshape(4, 3) + 1.0
    ids_a, mask_a = np.array([[0, 2, 2], [3, 1, 0]]), np.array([[1, 1, 1], [0, 0, 0]])
    ids_b, mask_b = np.array([[1, 1], [2, 0]]), np.array([[0, 0], [1, 0]])
    j = bow_ref.bag_mean(table, ids_a, mask_a, ids_b, mask_b)
    assert torch.equal(j[0], (table[0] + 2 * table[2]) / 3) and torch.equal(j[1], table[2])
    a, b = bow_ref.bag_mean(table, ids_a, mask_a, ids_b, mask_b, separate=True)
    assert torch.equal(a[1], table[3]) and torch.equal(b[0], table[1]) and torch.equal(b[1], table[2])
    assert mask_a[1, 0] == 0                                   # the restatement leaves its inputs alone


def test_entry_points_are_declared_listed_and_exported():
    from nnr_amd import _lib, profile
    header = open(os.path.join(ROOT, 'include', 'nnr_hip.h')).read()
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert (L.nnr_tape_fn_id(name.encode()) >= 0) == (name != 'nnr_bag_mean_bwd_ws_floats'), name
    assert L.nnr_bag_mean_bwd_ws_floats(0) == 0 and L.nnr_bag_mean_bwd_ws_floats(33) == 2 * 2 * 320
    assert profile.HBM_KERNELS_OTHER['bag_mean_fwd'] == (('bag_mean_fwd_kernel',), 1)
    assert profile.HBM_KERNELS_OTHER['bag_mean_bwd'] == (('bag_mean_bwd_kernel', 'bag_mean_bwd_fix_kernel'), 2)
    assert open(os.path.join(ROOT, 'nnr_amd', 'csrc', 'build.sh')).read().count(' bag;') == 1
