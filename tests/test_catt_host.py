"""CPU checks of the CATT user encoder / candidate-attention layers: the float64 restatement the GPU tests compare against is pinned to
the reference's own results (tests/golden/*CATT*.npz, layer_cand_attn.npz), the model constructs with the reference's parameter
names and shapes, and the new entry points are exported."""
import ctypes
import os

import numpy as np
import pytest
import torch

from cand_attn_ref import concat_form, pq_form, catt_user_rep, f64
from golden_io import GoldenCase, GOLDEN_DIR
from golden_weights import make_state

CATT_CASES = ['tiny_CNE_CATT_stable', 'tiny_CNN_CATT', 'full_CNE_CATT_g1p0_stable']


def _catt_state(case):
    D, A = case.expect('hist_rep').shape[-1], int(case.config.attention_dim)
    shapes = {'user_encoder.affine1.weight': (A, 2 * D), 'user_encoder.affine1.bias': (A,), 'user_encoder.affine2.weight': (1, A),
              'user_encoder.affine2.bias': (1,)}
    return make_state(shapes, case.meta['seed'], case.meta['gain'])      # (per-name generators: a subset of the names gives the same arrays)


@pytest.mark.parametrize('tag', CATT_CASES)
def test_restatement_reproduces_the_reference_user_representation(tag):
    case = GoldenCase(tag)
    got = catt_user_rep(case.expect('hist_rep'), case.expect('cand_rep'), case.expect('in/user_history_mask'), _catt_state(case))
    err = float((got - f64(case.expect('user_rep'))).abs().max())
    print('%s: restatement vs reference user_rep %.3e' % (tag, err))
    assert err <= 1e-6


def test_the_tiny_fixture_holds_users_without_history():
    lens = GoldenCase('tiny_CNE_CATT_stable').expect('in/user_history_mask').astype(bool).sum(axis=1)
    assert int((lens == 0).sum()) >= 2 and int(lens.max()) >= 4


@pytest.mark.parametrize('kind', ['single', 'multi'])
@pytest.mark.parametrize('mtag', ['mask', 'nomask'])
def test_restatement_reproduces_the_reference_layers(kind, mtag):
    z = np.load(os.path.join(GOLDEN_DIR, 'layer_cand_attn.npz'))
    par = {k: f64(z['%s/param/%s' % (kind, k)]).requires_grad_() for k in ('feature_affine.weight', 'query_affine.weight', 'query_affine.bias',
                                                                          'attention_affine.weight')}
    feat, query = f64(z['feature']).requires_grad_(), f64(z[kind + '/query']).requires_grad_()
    q3 = query.unsqueeze(1) if kind == 'single' else query
    W1 = torch.cat([par['query_affine.weight'], par['feature_affine.weight']], dim=1)
    mask = torch.from_numpy(z['mask']) if mtag == 'mask' else None
    _, out = concat_form(feat, q3, W1, par['query_affine.bias'], par['attention_affine.weight'].reshape(-1), 0.0, mask, 'tanh')
    out = out.squeeze(1) if kind == 'single' else out
    out.square().sum().backward()
    pre = '%s/%s/' % (kind, mtag)
    assert float((out.detach() - f64(z[pre + 'out'])).abs().max()) <= 1e-6
    assert float((feat.grad - f64(z[pre + 'grad/feature'])).abs().max()) <= 1e-6
    assert float((query.grad - f64(z[pre + 'grad/query'])).abs().max()) <= 1e-6
    for k, p in par.items():
        assert float((p.grad - f64(z[pre + 'grad/param/' + k])).abs().max()) <= 1e-6, k


def test_projection_form_equals_the_concat_form():
    g = torch.Generator().manual_seed(3)
    B, N, H, A, D = 3, 2, 5, 6, 7
    feat, query = torch.randn(B, H, D, generator=g).double(), torch.randn(B, N, D, generator=g).double()
    W1, b1, w2 = torch.randn(A, 2 * D, generator=g).double(), torch.randn(A, generator=g).double(), torch.randn(A, generator=g).double()
    mask = torch.tensor([[0] * 5, [1] * 5, [1, 1, 0, 0, 0]])
    for act in ('relu', 'tanh'):
        for m in (mask, None):
            a0, o0 = concat_form(feat, query, W1, b1, w2, 0.3, m, act)
            a1, o1 = pq_form(query @ W1[:, :D].t() + b1, feat @ W1[:, D:].t(), w2, feat, m, act)
            assert float((a0 - a1).abs().max()) <= 1e-12 and float((o0 - o1).abs().max()) <= 1e-12


@pytest.mark.parametrize('tag', CATT_CASES)
def test_model_constructs_with_the_reference_parameters(tag):
    """Fails without the feature: Model raises for user_encoder='CATT'."""
    from nnr_amd import config
    from nnr_amd.model import Model
    from nnr_amd.user_encoders import CATT
    assert 'CATT' in config.USER_ENCODERS
    case = GoldenCase(tag)
    model = Model(case.config, case.word_table())
    assert type(model.user_encoder) is CATT and model.model_name.endswith('-CATT')
    case.load_into(model)                                    # names and shapes equal the reference's named_parameters()
    D, A = model.news_embedding_dim, int(case.config.attention_dim)
    sd = model.user_encoder.state_dict()
    assert tuple(sd['affine1.weight'].shape) == (A, 2 * D) and tuple(sd['affine2.weight'].shape) == (1, A) and tuple(sd['affine2.bias'].shape) == (1,)
    model.initialize()
    assert float(model.user_encoder.affine1.bias.abs().max()) == 0.0 and float(model.user_encoder.affine2.bias.abs().max()) == 0.0


def test_an_unknown_user_encoder_still_raises():
    from nnr_amd.model import Model
    from nnr_amd.config import make_config
    cfg = make_config(['--user_encoder=LSTUR'], corpus_sizes=dict(vocabulary_size=50))
    with pytest.raises(Exception, match='CATT'):
        Model(cfg)


def test_layers_keep_the_reference_state_dict_names():
    from nnr_amd.layers import CandidateAttention, MultipleCandidateAttention
    z = np.load(os.path.join(GOLDEN_DIR, 'layer_cand_attn.npz'))
    for kind, cls in (('single', CandidateAttention), ('multi', MultipleCandidateAttention)):
        mod = cls(24, 24, 12)
        mod.initialize()
        assert list(mod.state_dict().keys()) == [str(k) for k in z[kind + '/param_names']]
        for k, v in mod.state_dict().items():
            assert tuple(v.shape) == tuple(z['%s/param/%s' % (kind, k)].shape)


def test_entry_points_are_listed_and_exported():
    from nnr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('nnr_cand_attn_ws_floats', 'nnr_cand_attn_fwd', 'nnr_cand_attn_bwd'):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    L = _lib.lib()
    assert L.nnr_tape_fn_id(b'nnr_cand_attn_fwd') >= 0 and L.nnr_tape_fn_id(b'nnr_cand_attn_bwd') >= 0 and L.nnr_tape_fn_id(b'nnr_cand_attn_ws_floats') < 0
    slots = L.nnr_slot_workspace_floats(200)
    assert L.nnr_cand_attn_ws_floats(64, 5, 50, 200) == 64 * 5 * 50 + 64 * 5 * 200 + slots
    assert L.nnr_cand_attn_ws_floats(0, 5, 50, 200) < 0


def test_profile_tooling_knows_the_kernels():
    from nnr_amd import profile
    assert profile.HBM_KERNELS_OTHER['cand_attn_fwd'][0] == ('cand_attn_fwd_kernel',)
    assert profile.HBM_KERNELS_OTHER['cand_attn_bwd'] == (('cand_attn_bwd_da_kernel', 'cand_attn_bwd_dx_kernel'), 2)
    assert not set(profile.HBM_KERNELS_OTHER) & set(profile.HBM_KERNELS)
