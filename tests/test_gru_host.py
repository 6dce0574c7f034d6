"""Host tests of the GRU user encoder (DAE-GRU): the float64 restatement tests/gru_ref.py against torch.nn.GRU on a PackedSequence through
the reference's sort / drop-empties / de-sort path, the public surface (dispatch, names, shapes, initialisation, refusals), the host mirror
of the packed / fragment layouts, and what the fixtures must contain."""
import numpy as np
import pytest
import torch

import gru_ref
from golden_io import GoldenCase

TINY = ['tiny_DAE_GRU', 'tiny_CNN_GRU', 'tiny_CNE_GRU_h48']
SHAPES = [(5, 7, 12, 10, [7, 0, 3, 1, 7]), (19, 50, 100, 48, None), (33, 9, 20, 112, None), (16, 50, 300, 200, None), (3, 4, 6, 20, [0, 0, 0]),
          (64, 50, 300, 200, None)]


def _lens(B, T, lens, g):
    if lens is not None:
        return torch.tensor(lens)
    out = torch.randint(0, T + 1, (B,), generator=g)
    out[0], out[1] = 0, T
    return out


@pytest.mark.parametrize('with_h0', [False, True], ids=['zero_start', 'h0'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s[:4])))
def test_restatement_equals_nn_gru_on_a_packed_sequence(shape, with_h0):
    B, T, D, H, lens = shape
    g = torch.Generator().manual_seed(B * 1000 + T)
    gru = torch.nn.GRU(D, H, batch_first=True).double()
    x = torch.randn(B, T, D, generator=g, dtype=torch.float64)
    lens = _lens(B, T, lens, g)
    mask = gru_ref.prefix_mask(lens, T)
    mask = torch.stack([row[torch.randperm(T, generator=g)] for row in mask])          # only the count matters
    h0 = torch.randn(B, H, generator=g, dtype=torch.float64) if with_h0 else None
    with torch.no_grad():
        exp = gru_ref.packed_path(x, mask, gru, h0)
        p = [t.detach() for t in (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)]
        hs, got = gru_ref.gru_frozen(x, gru_ref.lengths(mask), *p, h0=h0)
    assert float((got - exp).abs().max()) <= 1e-13
    assert torch.equal(gru_ref.lengths(mask), lens)
    for b in range(B):
        n = int(lens[b])
        assert float(hs[b, n:].abs().sum()) == 0.0
        if n:
            assert torch.equal(hs[b, n - 1], got[b])
        elif with_h0:
            assert torch.equal(got[b], h0[b])
        else:
            assert float(got[b].abs().max()) == 0.0


def _cfg(**over):
    from nnr_amd import config
    kw = dict(news_encoder='CNN', user_encoder='GRU', vocabulary_size=30, word_embedding_dim=8, cnn_kernel_num=12, hidden_dim=10, max_history_num=6)
    kw.update(over)
    return config.make_config([], **kw)


def _model(cfg):
    from nnr_amd.model import Model
    return Model(cfg, torch.zeros(cfg.vocabulary_size, cfg.word_embedding_dim))


def test_dispatch_state_dict_and_flat_lists():
    from nnr_amd import config, user_encoders, layers, step
    m = _model(_cfg())
    ue = m.user_encoder
    assert type(ue) is user_encoders.GRU and ue.news_encoder is m.news_encoder and m.model_name == 'CNN-GRU'
    assert isinstance(ue.gru, layers.GRUParams) and hasattr(ue, 'encode_user')
    D, H = m.news_embedding_dim, 10
    own = {k: tuple(v.shape) for k, v in ue.state_dict().items() if not k.startswith('news_encoder.')}
    assert own == {'gru.weight_ih_l0': (3 * H, D), 'gru.weight_hh_l0': (3 * H, H), 'gru.bias_ih_l0': (3 * H,), 'gru.bias_hh_l0': (3 * H,),
                   'dec.weight': (D, H), 'dec.bias': (D,)}
    ref = torch.nn.GRU(D, H, batch_first=True)
    assert list(ue.gru.state_dict()) == list(ref.state_dict())
    ue.gru.load_state_dict(ref.state_dict(), strict=True)
    assert step.kind(m) is None
    assert config.ALL_USER_ENCODERS == config.USER_ENCODERS + ['GRU']
    assert config.ALL_USER_ENCODERS == ['SUE', 'MHSA', 'ATT', 'CATT', 'OMAP', 'PUE', 'FIM', 'GRU']


def test_initialize_is_the_references():
    torch.manual_seed(3)
    m = _model(_cfg(hidden_dim=48, cnn_kernel_num=20))
    m.initialize()
    ue = m.user_encoder
    for w in (ue.gru.weight_ih_l0, ue.gru.weight_hh_l0):
        w = w.detach().double()
        gram = w.t() @ w if w.shape[0] >= w.shape[1] else w @ w.t()          # orthogonal_ on the WHOLE [3H, .] matrix
        assert float((gram - torch.eye(gram.shape[0], dtype=torch.float64)).abs().max()) <= 1e-5
    for b in (ue.gru.bias_ih_l0, ue.gru.bias_hh_l0, ue.dec.bias):
        assert float(b.detach().abs().max()) == 0.0
    w = ue.dec.weight.detach()
    bound = torch.nn.init.calculate_gain('tanh') * (6.0 / (w.shape[0] + w.shape[1])) ** 0.5
    assert float(w.abs().max()) <= bound and float(w.abs().max()) >= 0.9 * bound
    assert abs(float(w.std()) - bound / 3 ** 0.5) <= 0.1 * bound


def test_refusals():
    with pytest.raises(Exception, match='LSTUR is not on the MI355X hot path .*CATT, FIM, OMAP, PUE, GRU'):
        _model(_cfg(user_encoder='LSTUR'))
    for over in (dict(hidden_dim=257), dict(hidden_dim=0), dict(max_history_num=256)):
        with pytest.raises(Exception, match='unsupported size'):
            _model(_cfg(**over))
    _model(_cfg(hidden_dim=256, max_history_num=255))
    _model(_cfg(hidden_dim=1))


def test_host_mirror_of_the_rule_is_the_librarys():
    from nnr_amd import ops, _lib
    for H, T in ((0, 5), (1, 1), (10, 7), (200, 50), (256, 255), (257, 50), (200, 256), (200, 0)):
        assert ops.gru_supported(H, T) == (_lib.lib().nnr_gru_dims(H, T, None, None, None) == 0), (H, T)
    assert ops.gru_dims(200, 50) == (13, 208, 832) and ops.gru_dims(10, 7) == (1, 16, 64)


@pytest.mark.parametrize('H,D', [(10, 12), (48, 100), (112, 20), (200, 300), (1, 3), (256, 8), (17, 5)])
def test_packed_layouts_round_trip(H, D):
    from nnr_amd import ops
    g = torch.Generator().manual_seed(H)
    w_ih, w_hh = torch.randn(3 * H, D, generator=g), torch.randn(3 * H, H, generator=g)
    b_ih, b_hh = torch.randn(3 * H, generator=g), torch.randn(3 * H, generator=g)
    w_ihp, b_p, wf, wb = ops.gru_pack_host(w_ih, w_hh, b_ih, b_hh)
    UB = (H + 15) // 16
    assert tuple(w_ihp.shape) == (UB * 64, D) and wf.numel() == UB * 3 * UB * 256 and wb.numel() == UB * UB * 4 * 256
    back_f, full_f = gru_ref.unpack_forward_fragments(wf, H)
    back_b, rows_b = gru_ref.unpack_backward_fragments(wb, H)
    assert torch.equal(back_f, w_hh) and torch.equal(back_b, w_hh)
    unit = torch.arange(H)
    for s in range(3):
        assert torch.equal(w_ihp[gru_ref.p_index(unit, s)], w_ih[s * H:(s + 1) * H])
    assert float(w_ihp[gru_ref.p_index(unit, 3)].abs().max()) == 0.0 and float(rows_b[gru_ref.p_index(unit, 2)].abs().max()) == 0.0
    assert torch.equal(b_p[gru_ref.p_index(unit, 0)], b_ih[:H] + b_hh[:H]) and torch.equal(b_p[gru_ref.p_index(unit, 1)], b_ih[H:2 * H] + b_hh[H:2 * H])
    assert torch.equal(b_p[gru_ref.p_index(unit, 2)], b_ih[2 * H:]) and torch.equal(b_p[gru_ref.p_index(unit, 3)], b_hh[2 * H:])      # b_hn is NOT folded
    # everything that is not a live (unit, k) is zero padding
    assert int(full_f.count_nonzero()) == int(w_hh.count_nonzero()) and int(w_ihp.count_nonzero()) == int(w_ih.count_nonzero())
    assert int(rows_b.count_nonzero()) == int(w_hh.count_nonzero()) and int(b_p.count_nonzero()) == 4 * H


@pytest.mark.parametrize('tag', TINY)
def test_tiny_fixtures_hold_an_empty_and_a_full_user_and_visible_biases(tag):
    case = GoldenCase(tag)
    mask = case.expect('in/user_history_mask').astype(bool)
    lens = mask.sum(axis=1)
    assert (lens == 0).any() and (lens == mask.shape[1]).any(), lens
    shapes = {k: tuple(p.shape) for k, p in _model_of(case).named_parameters()}
    st = case.initial_state(shapes)
    assert float(np.abs(np.tanh(st['user_encoder.dec.bias'])).max()) > 1e-2
    for k in ('gru.bias_ih_l0', 'gru.bias_hh_l0'):
        assert float(np.abs(st['user_encoder.' + k]).max()) > 1e-2
    user = case.expect('user_rep')
    assert float(np.abs(user[lens == 0]).max()) == 0.0 and float(np.abs(user[lens > 0]).max()) > 1e-2


def _model_of(case):
    from nnr_amd.model import Model
    return Model(case.config, case.word_table())


@pytest.mark.parametrize('tag', TINY + ['full_DAE_GRU_g1p0'])
def test_restatement_gives_the_fixtures_user_representation(tag):
    """The reference's own fp32 run (history representation in, user representation out) against the float64 restatement on the fixture's weights."""
    case = GoldenCase(tag)
    shapes = {k: tuple(p.shape) for k, p in _model_of(case).named_parameters()}
    st = case.initial_state(shapes)
    D, H = st['user_encoder.dec.weight'].shape
    assert H == case.config.hidden_dim and (tag != 'tiny_CNE_GRU_h48' or (H, D) == (48, 292)) and (tag != 'full_DAE_GRU_g1p0' or (H, D) == (200, 300))
    exp = case.expect('user_rep')
    got = gru_ref.gru_user_rep(case.expect('hist_rep'), case.expect('in/user_history_mask'), st)
    assert float((got.unsqueeze(1) - torch.from_numpy(exp).double()).abs().max()) <= 2e-6
