"""Host tests of the FIM baseline (HDC news encoder, FIM user encoder, FIM click head): the float64 restatement tests/fim_ref.py against
the reference's own float64 run stored in the fixtures, the fixtures' margin condition, and the public surface -- flags, dispatch, the
reference's assertions, refusals, parameter names and shapes, and the paths this pair does not take."""
import functools

import numpy as np
import pytest
import torch

import fim_ref
from golden_io import GoldenCase, eval_fixture
from nnr_amd.synth import BATCH_FIELDS

TINY = ['tiny_HDC_FIM', 'tiny_HDC_FIM_p3']
FULL = 'full_HDC_FIM_g1p0'
MARGIN_FACTOR = 20.0
FLAGS = dict(HDC_window_size=3, HDC_filter_num=150, conv3D_filter_num_first=32, conv3D_kernel_size_first=3, conv3D_filter_num_second=16,
             conv3D_kernel_size_second=3, maxpooling3D_size=3, maxpooling3D_stride=3)


def _model(cfg, table=None):
    from nnr_amd.model import Model
    return Model(cfg, table if table is not None else torch.zeros(cfg.vocabulary_size, cfg.word_embedding_dim))


@functools.lru_cache(maxsize=None)
def restated(tag):
    """The float64 restatement on a fixture's weights and batch, with its gradients: computed once per fixture."""
    case = GoldenCase(tag)
    shapes = {k: tuple(p.shape) for k, p in _model(case.config, case.word_table()).named_parameters()}
    st = fim_ref.leaf_state(case.initial_state(shapes))
    out = fim_ref.model(st, {k: case.expect('in/' + k) for k in BATCH_FIELDS}, case.config)
    out['loss'].backward()
    return case, st, out


def fixture_margin(case):
    """(M, smallest margin over both layers) of a tiny fixture, see tools/make_goldens.py:fim_margin."""
    P, St = case.config.maxpooling3D_size, case.config.maxpooling3D_stride
    worst = min(fim_ref.pool_margins(case.expect('f64/fim/' + k), P, St)[0] for k in ('za', 'zb'))
    return MARGIN_FACTOR * float(case.expect('fim/conv_dev')), worst


@pytest.mark.parametrize('tag', TINY)
def test_restatement_matches_the_reference_float64_run(tag):
    case, st, out = restated(tag)
    pairs = [('logits', out['logits']), ('loss', out['loss']), ('fim/za', out['za']), ('fim/zb', out['zb']),
             ('cand_rep/d0', out['cand_d0']), ('cand_rep/dL', out['cand_dL']), ('hist_rep/d0', out['hist_d0']), ('hist_rep/dL', out['hist_dL'])]
    pairs += [('grad/' + k, v.grad) for k, v in st.items()]
    for name, got in pairs:
        exp = np.asarray(case.expect('f64/' + name), dtype=np.float64)
        err, s = float(np.abs(got.detach().numpy().reshape(exp.shape) - exp).max()), float(np.abs(exp).max())
        assert err <= 1e-6 * max(s, 1e-30), (name, err, s)
    a1 = fim_ref.lowest_argmax(fim_ref.windows(torch.from_numpy(case.expect('f64/fim/za')), case.config.maxpooling3D_size, case.config.maxpooling3D_stride))
    assert torch.equal(a1, out['a1'])


def test_restatement_matches_the_full_size_fixture():
    """The full-size fixture holds the reference's fp32 run only: logits and loss within 1e-5 of their scale (the fp32 run's own distance
    from float64 in the tiny fixtures is below 1e-6), every stored gradient element within 1e-4 of the tensor's float64 scale."""
    case, st, out = restated(FULL)
    for name in ('logits', 'loss'):
        exp = np.asarray(case.expect(name), dtype=np.float64)
        err, s = float(np.abs(out[name].detach().numpy() - exp).max()), float(np.abs(exp).max())
        assert err <= 1e-5 * s, (name, err, s)
    for k, v in st.items():
        exp, act = case.expect_grad(k, v.grad)
        s = float(v.grad.abs().max()) if k != 'fc.bias' else float(st['fc.weight'].grad.abs().max())
        assert float(np.abs(act - exp.astype(np.float64)).max()) <= 1e-4 * s, k


@pytest.mark.parametrize('tag', TINY)
def test_fixture_margin_condition(tag):
    """Every pool maximum of the float64 run beats every competitor not exactly equal to it by M = 20 x the reference's own fp32 deviation."""
    case = GoldenCase(tag)
    M, worst = fixture_margin(case)
    dev = float(case.expect('fim/conv_dev'))
    print('%s: fp32 deviation %.2e, M %.2e, smallest margin %.2e' % (tag, dev, M, worst))
    assert 1e-8 < dev < 2e-6 and worst >= M


def test_tiny_fixture_drops_a_remainder_and_p3_is_minimal():
    case = GoldenCase(TINY[0])
    assert case.expect('f64/fim/za').shape[2:] == (9, 10, 10) and case.expect('f64/fim/zb').shape[2:] == (2, 3, 3)
    p3 = GoldenCase(TINY[1])
    assert p3.expect('f64/fim/za').shape[2:] == (15, 17, 17) and fim_ref.pool_sizes(19, 17, p3.config) == (1, 1, 1)
    assert fim_ref.pool_sizes(19, 16, p3.config)[0] == 0
    full = GoldenCase(FULL)
    assert fim_ref.pool_sizes(34, 50, full.config) == (4, 2, 2) and full.expect('user_rep').shape == (2, 5, 256)


def test_flags_defaults_and_list_orders():
    from nnr_amd import config
    cfg = config.make_config([])
    for k, v in FLAGS.items():
        assert getattr(cfg, k) == v, k
    cfg = config.make_config(['--news_encoder', 'HDC', '--user_encoder', 'FIM', '--click_predictor', 'FIM', '--HDC_filter_num', '8', '--maxpooling3D_stride', '4'])
    assert (cfg.HDC_filter_num, cfg.maxpooling3D_stride, cfg.click_predictor) == (8, 4, 'FIM')
    assert config.NEWS_ENCODERS == ['CNE', 'CNN', 'MHSA', 'PNE', 'DAE', 'Inception', 'HDC', 'KCNN']
    assert config.USER_ENCODERS == ['SUE', 'MHSA', 'ATT', 'CATT', 'OMAP', 'PUE', 'FIM']


def _cfg(**over):
    from nnr_amd import config
    kw = dict(news_encoder='HDC', user_encoder='FIM', click_predictor='FIM', vocabulary_size=30, word_embedding_dim=8, max_title_length=17,
              max_history_num=17, HDC_filter_num=6, conv3D_filter_num_first=3, conv3D_filter_num_second=2)
    kw.update(over)
    return config.make_config([], **kw)


def test_dispatch_and_head():
    from nnr_amd import news_encoders, user_encoders
    m = _model(_cfg())
    assert type(m.news_encoder) is news_encoders.HDC and type(m.user_encoder) is user_encoders.FIM and m.user_encoder.news_encoder is m.news_encoder
    assert m.news_embedding_dim is None and m.click_predictor == 'FIM' and m.model_name == 'HDC-FIM'
    assert tuple(m.fc.weight.shape) == (1, 2) and m.news_encoder.category_embedding.weight.shape[1] == 8
    m = _model(_cfg(max_title_length=32, max_history_num=50, conv3D_filter_num_second=16))
    assert tuple(m.fc.weight.shape) == (1, 256)
    m.initialize()
    assert float(m.fc.bias.detach().abs().max()) == 0.0


def test_pairing_assertions_and_refusals():
    from nnr_amd import news_encoders, user_encoders
    cnn = _cfg(news_encoder='CNN')
    with pytest.raises(AssertionError, match='For FIM, the news encoder must be HDC'):
        user_encoders.FIM(news_encoders.CNN(cnn, torch.zeros(30, 8)), cnn)
    with pytest.raises(AssertionError, match='HDC and FIM must be paired and can not be used alone'):
        _model(cnn)
    with pytest.raises(AssertionError, match='HDC and FIM must be paired and can not be used alone'):
        _model(_cfg(user_encoder='ATT'))
    with pytest.raises(AssertionError, match="For the model FIM, the click predictor must be specially set as 'FIM'"):
        _model(_cfg(click_predictor='dot_product'))
    with pytest.raises(Exception, match='out of scope'):
        _model(_cfg(news_encoder='CNN', user_encoder='ATT', click_predictor='FIM'))
    with pytest.raises(Exception, match='out of scope'):
        _model(_cfg(news_encoder='CNN', user_encoder='ATT', click_predictor='mlp'))
    with pytest.raises(Exception, match='NAML is not on the MI355X hot path .*HDC, PNE, DAE, Inception, KCNN'):
        _model(_cfg(news_encoder='NAML', user_encoder='ATT', click_predictor='dot_product'))
    with pytest.raises(Exception, match='LSTUR is not on the MI355X hot path .*CATT, FIM, OMAP, PUE'):
        _model(_cfg(news_encoder='CNN', user_encoder='LSTUR', click_predictor='dot_product'))
    for over in (dict(maxpooling3D_size=3, maxpooling3D_stride=2), dict(conv3D_kernel_size_first=5), dict(max_history_num=16),
                 dict(maxpooling3D_size=5, maxpooling3D_stride=5, max_history_num=60, max_title_length=60)):
        with pytest.raises(Exception, match='unsupported size'):
            _model(_cfg(**over))
    with pytest.raises(Exception, match='unsupported size'):          # the LDS limit: raised by the constructor, not by the first forward
        _model(_cfg(conv3D_filter_num_first=700))
    with pytest.raises(Exception, match='HDC_window_size'):
        _model(_cfg(HDC_window_size=5))


def test_state_dict_is_the_references():
    case = GoldenCase(TINY[0])
    m = _model(case.config, case.word_table())
    names = {k: tuple(p.shape) for k, p in m.named_parameters()}
    assert sorted(names) == sorted(k[len('param1/'):] for k in case.z.files if k.startswith('param1/'))
    for k, shape in names.items():
        assert shape == tuple(case.expect('param1/' + k).shape), k
    F, S, E = case.config.HDC_filter_num, case.config.max_title_length + 2, case.config.word_embedding_dim
    assert names['news_encoder.layer_norm2.weight'] == (F, S) and names['news_encoder.dilated_conv1.weight'] == (F, E, 3)
    assert names['news_encoder.subCategory_embedding.weight'][1] == E and names['user_encoder.conv_3D_a.weight'] == (3, 4, 3, 3, 3)
    eval_fixture('tiny_HDC_FIM')                                      # strict: unchanged names and shapes


def test_paths_not_taken():
    from nnr_amd import evaluate, step
    m = _model(_cfg())
    assert step.kind(m) is None
    assert evaluate.news_reps_cacheable(m) is False
