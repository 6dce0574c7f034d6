"""CPU checks of the OMAP user encoder: the float64 restatement the GPU tests compare against (tests/omap_ref.py) is pinned to the
reference's own results (tests/golden/*OMAP*.npz: user representation, loss with the auxiliary term, W's gradient), the fixtures hold
what they were built to hold, the model constructs with the reference's parameter names and shapes, the flags parse, and the new
entry points are exported."""
import ctypes
import os

import numpy as np
import pytest
import torch

from omap_ref import omap_form, regularizer, omap_user_rep, f64
from golden_io import GoldenCase
from golden_weights import make_state

OMAP_CASES = ['tiny_CNE_OMAP_stable', 'tiny_CNN_OMAP', 'full_CNE_OMAP_g0p35_stable']
ENTRY_POINTS = ('nnr_omap_ws_floats', 'nnr_omap_fwd', 'nnr_omap_bwd', 'nnr_omap_reg_fwd', 'nnr_omap_reg_bwd')


def _W(case):
    D, K = case.expect('hist_rep').shape[-1], int(case.config.OMAP_head_num)
    return make_state({'user_encoder.W': (D, K)}, case.meta['seed'], case.meta['gain'])['user_encoder.W']      # (per-name generators)


def _click_loss(logits):
    return (-torch.log_softmax(logits, dim=1).select(dim=1, index=0)).mean()


@pytest.mark.parametrize('tag', OMAP_CASES)
def test_restatement_reproduces_the_reference(tag):
    """user_rep within 1e-6 (the bar of tests/test_catt_host.py); the fixture's loss = click loss + the restatement's auxiliary term within
    1e-6; the restatement's dW (click part + regulariser part) within 1e-6 of max(1, max|grad|)."""
    case = GoldenCase(tag)
    W = f64(_W(case)).requires_grad_()
    hist, cand = f64(case.expect('hist_rep')), f64(case.expect('cand_rep'))
    mask = torch.from_numpy(case.expect('in/user_history_mask'))
    user = omap_form(hist, cand, W, mask)['out']
    err = float((user.detach() - f64(case.expect('user_rep'))).abs().max())
    click = _click_loss((user * cand).sum(dim=2))
    aux = regularizer(W, float(case.config.HiFi_Ark_regularizer_coefficient))
    lerr = abs(float((click + aux).detach()) - float(case.expect('loss')))
    aerr = abs(float(aux.detach()) - float(case.expect('auxiliary_loss')))
    (click + aux).backward()
    exp = f64(case.expect('grad/user_encoder.W'))
    got = W.grad if case.full_arrays else W.grad.reshape(-1)[:64]
    gerr = float((got.reshape(-1) - exp.reshape(-1)).abs().max())
    print('%s: user_rep %.3e, loss %.3e, auxiliary %.3e, dW %.3e (max|grad| %.3e)' % (tag, err, lerr, aerr, gerr, float(exp.abs().max())))
    assert err <= 1e-6
    assert lerr <= 1e-6 and aerr <= 1e-6
    assert gerr <= 1e-6 * max(1.0, float(exp.abs().max()))
    gn = float(W.grad.norm())
    assert abs(gn - float(case.expect('gradnorm/user_encoder.W'))) <= 1e-5 * max(1.0, gn)


def test_the_tiny_fixture_holds_users_without_history_and_padded_rows():
    lens = GoldenCase('tiny_CNE_OMAP_stable').expect('in/user_history_mask').astype(bool).sum(axis=1)
    assert len(lens) == 8 and int((lens == 0).sum()) >= 2 and int(lens.max()) >= 4
    assert int(((lens > 0) & (lens < 6)).sum()) >= 1                                        # live users with padded rows (beta = 1/K there)


@pytest.mark.parametrize('tag', OMAP_CASES)
def test_the_fixtures_make_the_auxiliary_term_and_its_gradient_count(tag):
    case = GoldenCase(tag)
    aux, loss = float(case.expect('auxiliary_loss')), float(case.expect('loss'))
    click = float(_click_loss(torch.from_numpy(case.expect('logits')).double()))
    assert abs((loss - aux) - click) <= 1e-5
    assert 0.05 * click <= aux <= 2.0 * click, (aux, click)
    assert float(case.expect('gradnorm/user_encoder.W')) >= 0.01 * float(case.expect('grad_total_norm'))
    assert int(case.config.OMAP_head_num) == 3 and float(case.config.HiFi_Ark_regularizer_coefficient) == 0.1


def test_masked_scores_pass_no_gradient_in_the_restatement():
    """Quirk 3 in the restatement itself: for a user without history alpha is 1/H and dX equals the gradient with alpha held constant."""
    g = torch.Generator().manual_seed(3)
    X, C, W = (0.5 * torch.randn(2, 5, 8, generator=g)).double(), (0.5 * torch.randn(2, 3, 8, generator=g)).double(), torch.randn(8, 3, generator=g).double()
    mask = torch.tensor([[0] * 5, [1, 1, 1, 0, 0]])
    x1, x2, x3 = (X.clone().requires_grad_() for _ in range(3))
    r = omap_form(x1, C, W, mask)
    r['out'].square().sum().backward()
    omap_form(x2, C, W, mask, detach_alpha=True)['out'].square().sum().backward()
    omap_form(x3, C, W, mask, unblocked=True)['out'].square().sum().backward()
    assert float((r['alpha'][0] - 0.2).abs().max()) <= 1e-15
    assert float((r['beta'][0] - 1.0 / 3).abs().max()) <= 1e-15 and float((r['beta'][1, 3:] - 1.0 / 3).abs().max()) <= 1e-15
    assert float((x1.grad[0] - x2.grad[0]).abs().max()) <= 1e-14 and float((x1.grad[1] - x2.grad[1]).abs().max()) > 1e-4
    assert float((x1.grad[0] - x3.grad[0]).abs().max()) > 1e-4 and float((x1.grad[1] - x3.grad[1]).abs().max()) <= 1e-14


def test_regularizer_gradient_is_zero_at_an_exactly_zero_norm():
    W = torch.zeros(6, 3, dtype=torch.float64)
    W[0, 0], W[2, 1], W[5, 2] = 1.0, 2.0, -1.0
    W.requires_grad_()
    e = regularizer(W, 0.1)
    e.backward()
    assert float(e) == 0.0 and float(W.grad.abs().max()) == 0.0


@pytest.mark.parametrize('tag', OMAP_CASES)
def test_model_constructs_with_the_reference_parameters(tag):
    """Fails without the feature: Model raises for user_encoder='OMAP'."""
    from nnr_amd import config
    from nnr_amd.model import Model
    from nnr_amd.user_encoders import OMAP
    assert 'OMAP' in config.USER_ENCODERS
    case = GoldenCase(tag)
    model = Model(case.config, case.word_table())
    assert type(model.user_encoder) is OMAP and model.model_name.endswith('-OMAP')
    case.load_into(model)                                    # names and shapes equal the reference's named_parameters()
    D, K = model.news_embedding_dim, int(case.config.OMAP_head_num)
    sd = {k: v for k, v in model.user_encoder.state_dict().items() if not k.startswith('news_encoder.')}
    assert list(sd) == ['W'] and tuple(sd['W'].shape) == (D, K)
    assert not list(model.user_encoder.buffers(recurse=False))          # J_k / I_k are plain attributes
    assert tuple(model.user_encoder.J_k.shape) == (K, K) and tuple(model.user_encoder.I_k.shape) == (K, K)
    assert model.user_encoder.auxiliary_loss is None and model.news_encoder.auxiliary_loss is None
    model.initialize()                                       # orthogonal_(W)
    w = model.user_encoder.W.detach().double()
    assert float((w.t() @ w - torch.eye(K, dtype=torch.float64)).abs().max()) <= 1e-5
    from nnr_amd import step
    model.train()
    assert not step.supported(model)                         # the autograd path: no native / replayed step for this pair


def test_flags_parse_with_the_reference_names_and_defaults():
    from nnr_amd.config import make_config
    cfg = make_config(['--user_encoder=OMAP', '--OMAP_head_num=4'], corpus_sizes=dict(vocabulary_size=50))
    assert cfg.user_encoder == 'OMAP' and cfg.OMAP_head_num == 4 and cfg.HiFi_Ark_regularizer_coefficient == 0.1
    cfg = make_config(['--HiFi_Ark_regularizer_coefficient=0.25'])
    assert cfg.OMAP_head_num == 3 and cfg.HiFi_Ark_regularizer_coefficient == 0.25


def test_an_unknown_user_encoder_still_raises():
    from nnr_amd.model import Model
    from nnr_amd.config import make_config
    cfg = make_config(['--user_encoder=LSTUR'], corpus_sizes=dict(vocabulary_size=50))
    with pytest.raises(Exception, match='OMAP'):
        Model(cfg)


def test_entry_points_are_listed_and_exported():
    from nnr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    L = _lib.lib()
    for name in ENTRY_POINTS[1:]:
        assert L.nnr_tape_fn_id(name.encode()) >= 0, name
    assert L.nnr_tape_fn_id(b'nnr_omap_ws_floats') < 0
    B, N, H, D, K = 64, 5, 50, 900, 3
    assert L.nnr_omap_ws_floats(B, N, H, D, K) == B * K * D + B * H * K + B * H * H + B * D * K      # (the backward pass's; the forward's is smaller)
    assert L.nnr_omap_ws_floats(0, N, H, D, K) == -1                                               # NNR_ERR_ARG
    assert L.nnr_omap_ws_floats(B, N, 97, D, K) == -3 and L.nnr_omap_ws_floats(B, N, H, D, 17) == -3   # NNR_ERR_UNSUPPORTED, before any launch


def test_profile_tooling_knows_the_kernels():
    from nnr_amd import profile
    assert profile.HBM_KERNELS_OTHER['omap_fwd'] == (('omap_alpha_kernel', 'omap_mix_kernel', 'omap_pool_kernel'), 3)
    assert profile.HBM_KERNELS_OTHER['omap_bwd'] == (('omap_bwd_pool_kernel', 'omap_bwd_dalpha_kernel', 'omap_bwd_dx_kernel',
                                                      'partial_rows_sum_kernel<true'), 4)
    assert not set(profile.HBM_KERNELS_OTHER) & set(profile.HBM_KERNELS)
    csrc = os.path.join(os.path.dirname(os.path.abspath(profile.__file__)), 'csrc')
    src = open(os.path.join(csrc, 'omap.hip')).read() + open(os.path.join(csrc, 'common.h')).read()      # (the shared fixed-order row sum)
    for names, _ in (profile.HBM_KERNELS_OTHER['omap_fwd'], profile.HBM_KERNELS_OTHER['omap_bwd']):
        for n in names:
            assert 'void %s(' % n.split('<')[0] in src, n
