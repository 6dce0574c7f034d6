"""Host tests of the user-encoder ablations SUE_wo_GCN / SUE_wo_HCA (variantEncoders.py:342-419): the float64 restatement
tests/sue_ablation_ref.py against itself (the two forms of the intra-cluster stage, the key bias that cannot matter) and against the fixtures
captured from the reference's own code, the claim about intraCluster_K.bias' gradient, the public surface, and what the fixtures must
contain."""
import numpy as np
import pytest
import torch

import sue_ablation_ref as R
from golden_io import GoldenCase

WO_GCN = ['tiny_CNN_SUE_wo_GCN', 'tiny_CNE_SUE_wo_GCN_stable', 'full_CNN_SUE_wo_GCN_g1p0']
WO_HCA = ['tiny_CNN_SUE_wo_HCA', 'tiny_CNE_SUE_wo_HCA_stable', 'full_CNN_SUE_wo_HCA_g1p0', 'tiny_CNN_SUE_wo_HCA_ln']
TINY = [t for t in WO_GCN + WO_HCA if t.startswith('tiny_')]


def _model_of(case):
    from nnr_amd.model import Model
    return Model(case.config, case.word_table())


def _state(case):
    return case.initial_state({k: tuple(p.shape) for k, p in _model_of(case).named_parameters()})


def _random_problem(B, N, H, C, D, A, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, c = r(B, H, D), r(B, N, D)
    cidx = torch.randint(0, C, (B, H), generator=g)
    return x, c, cidx, (r(A, D) / D ** 0.5, 0.3 * r(A), r(A, D) / D ** 0.5, 0.3 * r(A))


@pytest.mark.parametrize('shape', [(3, 2, 6, 4, 7, 5), (4, 5, 50, 19, 40, 10)], ids=lambda s: 'x'.join(map(str, s)))
def test_the_two_forms_of_the_intra_stage_agree_and_the_key_bias_cannot_matter(shape):
    B, N, H, C, D, A = shape
    x, c, cidx, (Wk, bk, Wq, bq) = _random_problem(*shape, seed=sum(shape))
    out = {}
    for form in ('keys', 'gemv'):
        out[form] = R.seg_softmax_pool(R.intra_scores(x, c, Wk, bk, Wq, bq, form), x, cidx, C)
    for a, b in zip(out['keys'], out['gemv']):
        assert float((a - b).abs().max()) <= 1e-12
    moved = R.seg_softmax_pool(R.intra_scores(x, c, Wk, bk + 3.0 * torch.randn(A, dtype=torch.float64), Wq, bq, 'keys'), x, cidx, C)
    for a, b in zip(out['keys'], moved):
        assert float((a - b).abs().max()) <= 1e-12
    # scatter semantics: weights sum to one inside every non-empty cluster, an empty cluster's feature row is exactly zero
    alpha, feat = out['gemv']
    onehot = torch.nn.functional.one_hot(cidx, C).double()
    sums = torch.einsum('bnh,bhc->bnc', alpha, onehot)
    present = onehot.sum(dim=1) > 0
    assert float((sums - present.unsqueeze(1).double()).abs().max()) <= 1e-12
    assert float(feat[(~present).unsqueeze(1).expand(-1, N, -1)].abs().sum()) == 0.0


@pytest.mark.parametrize('tag', WO_GCN + WO_HCA)
def test_restatement_gives_the_fixtures_user_representation(tag):
    """The reference's own fp32 run (history / candidate representations in, user representation out) against the float64 restatement."""
    case = GoldenCase(tag)
    st = _state(case)
    exp = torch.from_numpy(case.expect('user_rep')).double()
    hist, cand = case.expect('hist_rep'), case.expect('cand_rep')
    if tag in WO_GCN:
        got = [R.sue_wo_gcn(hist, cand, case.expect('in/user_history_category_mask'), case.expect('in/user_history_category_indices'), st, form=f)['user_rep']
               for f in ('keys', 'gemv')]
        assert float((got[0] - got[1]).abs().max()) <= 1e-12
        got = got[1]
    else:
        got = R.sue_wo_hca(hist, case.expect('in/user_history_graph'), st, cand.shape[1], case.config)['user_rep']
    err = float((got - exp).abs().max())
    print('%s: restatement vs the reference fp32 user_rep %.3e (max|user_rep| %.3f)' % (tag, err, float(exp.abs().max())))
    assert err <= 2e-6


@pytest.mark.parametrize('tag', ['tiny_CNN_SUE_wo_GCN', 'tiny_CNN_SUE_wo_HCA', 'tiny_CNN_SUE_wo_HCA_ln'])
def test_restatement_gradients_follow_the_references_float64_run(tag):
    """CNN's representations do not depend on the user encoder, so d loss / d user_rep can be rebuilt from the fixture: the restatement's
    parameter gradients against the `f64/grad` of the reference's own classes."""
    case = GoldenCase(tag)
    st = _state(case)
    hist, cand = case.expect('f64/hist_rep'), case.expect('f64/cand_rep')
    logits = torch.from_numpy(case.expect('f64/logits'))
    B = logits.shape[0]
    dlogits = torch.softmax(logits, dim=1)
    dlogits[:, 0] -= 1.0
    dout = (dlogits / B).unsqueeze(2) * torch.from_numpy(cand)
    if 'wo_GCN' in tag:
        res = R.sue_wo_gcn(hist, cand, case.expect('in/user_history_category_mask'), case.expect('in/user_history_category_indices'), st, dout=dout)
    else:
        res = R.sue_wo_hca(hist, case.expect('in/user_history_graph'), st, cand.shape[1], case.config, dout=dout)
    for k, g in res.items():
        if k.startswith('grad/') and not k.endswith('intraCluster_K.bias'):
            exp = torch.from_numpy(case.expect('f64/grad/user_encoder.' + k[5:]))
            assert float((g - exp).abs().max()) <= 1e-10 * max(1.0, float(exp.abs().max())), k


@pytest.mark.parametrize('tag', WO_GCN)
def test_the_key_bias_gradient_is_rounding_noise_in_the_reference_itself(tag):
    case = GoldenCase(tag)
    q = float(np.abs(case.expect('grad/user_encoder.intraCluster_Q.bias')).max())
    k = float(np.abs(case.expect('grad/user_encoder.intraCluster_K.bias')).max())
    print('%s: max|d intraCluster_K.bias| %.2e, max|d intraCluster_Q.bias| %.2e' % (tag, k, q))
    assert q > 0 and k < 1e-5 * q
    if tag.startswith('tiny_'):
        q64 = float(np.abs(case.expect('f64/grad/user_encoder.intraCluster_Q.bias')).max())
        assert float(np.abs(case.expect('f64/grad/user_encoder.intraCluster_K.bias')).max()) < 1e-12 * q64


def _cfg(**over):
    from nnr_amd import config
    kw = dict(news_encoder='CNN', user_encoder='SUE_wo_GCN', vocabulary_size=30, word_embedding_dim=8, cnn_kernel_num=12, max_history_num=6, category_num=3,
              attention_dim=8)
    kw.update(over)
    return config.make_config([], **kw)


def _model(cfg):
    from nnr_amd.model import Model
    return Model(cfg, torch.zeros(cfg.vocabulary_size, cfg.word_embedding_dim))


@pytest.mark.parametrize('tag', ['tiny_CNN_SUE_wo_GCN', 'tiny_CNE_SUE_wo_GCN_stable', 'tiny_CNN_SUE_wo_HCA', 'tiny_CNN_SUE_wo_HCA_ln', 'full_CNN_SUE_wo_HCA_g1p0'])
def test_dispatch_names_and_shapes_are_the_fixtures(tag):
    from nnr_amd import user_encoders, step, config
    case = GoldenCase(tag)
    m = _model_of(case)
    ue = m.user_encoder
    user = case.config.user_encoder
    assert type(ue) is getattr(user_encoders, user) and ue.news_encoder is m.news_encoder
    assert m.model_name == case.config.news_encoder + '-' + user and hasattr(ue, 'encode_user') and ue.needs_history_graph
    assert sorted(k for k, _ in m.named_parameters()) == sorted(case.param_names())
    if case.full_arrays:
        for k, p in m.named_parameters():
            assert tuple(p.shape) == tuple(case.expect('grad/' + k).shape), k
    assert step.kind(m) is None
    assert config.VARIANT_USER_ENCODERS == ['SUE_wo_GCN', 'SUE_wo_HCA']
    assert not set(config.VARIANT_USER_ENCODERS) & set(config.ALL_USER_ENCODERS)


def test_parameter_surface_of_both_encoders():
    m = _model(_cfg())
    D = m.news_embedding_dim
    A = max(8, D // 4)
    own = {k: tuple(v.shape) for k, v in m.user_encoder.state_dict().items() if not k.startswith('news_encoder.')}
    assert own == {'intraCluster_K.weight': (A, D), 'intraCluster_K.bias': (A,), 'intraCluster_Q.weight': (A, D), 'intraCluster_Q.bias': (A,),
                   'clusterFeatureAffine.weight': (D, D), 'clusterFeatureAffine.bias': (D,), 'interClusterAttention.K.weight': (A, D),
                   'interClusterAttention.Q.weight': (A, D), 'interClusterAttention.Q.bias': (A,)}
    assert m.user_encoder.category_num == 4 and m.user_encoder.attention_dim == A
    m = _model(_cfg(user_encoder='SUE_wo_HCA', gcn_layer_num=2))
    own = {k: tuple(v.shape) for k, v in m.user_encoder.state_dict().items() if not k.startswith('news_encoder.')}
    assert own == {'proxy_node_embedding': (3, D), 'gcn.gcn_layers.0.W.weight': (D, D), 'gcn.gcn_layers.0.W.bias': (D,), 'gcn.gcn_layers.1.W.weight': (D, D),
                   'gcn.gcn_layers.1.W.bias': (D,), 'attention.affine1.weight': (8, D), 'attention.affine1.bias': (8,), 'attention.affine2.weight': (1, 8)}


def test_initialize_is_the_references():
    torch.manual_seed(5)
    m = _model(_cfg(cnn_kernel_num=60))
    with torch.no_grad():
        for p in m.user_encoder.parameters():
            p.fill_(7.0)
    m.initialize()
    ue = m.user_encoder
    for b in (ue.intraCluster_K.bias, ue.intraCluster_Q.bias, ue.clusterFeatureAffine.bias, ue.interClusterAttention.Q.bias):
        assert float(b.detach().abs().max()) == 0.0
    for w, gain in ((ue.intraCluster_K.weight, 1.0), (ue.intraCluster_Q.weight, 1.0), (ue.clusterFeatureAffine.weight, 2.0 ** 0.5),
                    (ue.interClusterAttention.K.weight, 1.0), (ue.interClusterAttention.Q.weight, 1.0)):
        w = w.detach()
        bound = gain * (6.0 / (w.shape[0] + w.shape[1])) ** 0.5
        assert 0.9 * bound <= float(w.abs().max()) <= bound
    m = _model(_cfg(user_encoder='SUE_wo_HCA', cnn_kernel_num=60))
    with torch.no_grad():
        for p in m.user_encoder.parameters():
            p.fill_(7.0)
    m.initialize()
    ue = m.user_encoder
    assert float(ue.proxy_node_embedding.detach().abs().max()) == 0.0 and float(ue.attention.affine1.bias.detach().abs().max()) == 0.0
    for w, gain in [(l.W.weight, 2.0 ** 0.5) for l in ue.gcn.gcn_layers] + [(ue.attention.affine1.weight, 5.0 / 3), (ue.attention.affine2.weight, 1.0)]:
        w = w.detach()
        bound = gain * (6.0 / (w.shape[0] + w.shape[1])) ** 0.5
        assert 0.8 * bound <= float(w.abs().max()) <= bound * (1 + 1e-6)
    for l in ue.gcn.gcn_layers:
        assert float(l.W.bias.detach().abs().max()) == 0.0


def test_refusals_end_with_the_new_names_and_sizes_are_refused():
    for over in (dict(user_encoder='LSTUR'), dict(news_encoder='NAML')):
        with pytest.raises(Exception, match=r'is not on the MI355X hot path .*SUE_wo_GCN, SUE_wo_HCA\)$'):
            _model(_cfg(**over))
    for over in (dict(max_history_num=65), dict(category_num=32), dict(negative_sample_num=8)):
        with pytest.raises(Exception, match='unsupported size'):
            _model(_cfg(**over))
    _model(_cfg(max_history_num=64, category_num=31, negative_sample_num=7))
    _model(_cfg(user_encoder='SUE_wo_HCA', max_history_num=65, category_num=40))        # (no segmented pool there)


def test_host_mirror_of_the_rule_is_the_librarys():
    """Null pointers: the size rule answers before the pointers are looked at, and nothing is launched."""
    from nnr_amd import ops, _lib
    lib = _lib.lib()
    for B, N, Hn, C, D in ((1, 1, 1, 1, 1), (64, 5, 50, 19, 900), (2, 8, 64, 32, 33), (2, 9, 64, 32, 33), (2, 8, 65, 32, 33), (2, 8, 64, 33, 33),
                           (2, 0, 6, 4, 8), (2, 2, 0, 4, 8), (2, 2, 6, 0, 8), (2, 2, 6, 4, 0), (0, 2, 6, 4, 8)):
        want = ops.seg_pool_supported(Hn, C, N, D, B)
        rc_f = lib.nnr_sue_seg_pool_fwd(None, None, None, B, N, Hn, C, D, 1.0, None, None, None)
        rc_b = lib.nnr_sue_seg_pool_bwd(None, None, None, None, None, B, N, Hn, C, D, 1.0, None, None, None, None)
        assert (rc_f != _lib.NNR_ERR_UNSUPPORTED) == want and (rc_b != _lib.NNR_ERR_UNSUPPORTED) == want, (B, N, Hn, C, D)
        assert rc_f != 0 and rc_b != 0                     # (a supported size with null pointers is an argument error, not a launch)
        # the keys pair (nnr_sue_intra_*) answers by the same rule, plus A >= 1
        assert rc_f == rc_b == (_lib.NNR_ERR_ARG if want else _lib.NNR_ERR_UNSUPPORTED)
        for A in (0, 1, 230):
            for rc in (lib.nnr_sue_intra_fwd(None, None, None, None, B, N, Hn, C, A, D, None, None, None),
                       lib.nnr_sue_intra_bwd(None, None, None, None, None, None, B, N, Hn, C, A, D, None, None, None, None, None)):
                assert rc == (_lib.NNR_ERR_ARG if want and A >= 1 else _lib.NNR_ERR_UNSUPPORTED), (B, N, Hn, C, A, D)
    assert (ops.SEG_POOL_MAXH, ops.SEG_POOL_MAXC, ops.SEG_POOL_MAXN) == (64, 32, 8)


@pytest.mark.parametrize('tag', TINY)
def test_tiny_fixtures_meet_their_conditions(tag):
    case = GoldenCase(tag)
    hm = case.expect('in/user_history_mask').astype(bool)
    cidx = case.expect('in/user_history_category_indices')
    cmask = case.expect('in/user_history_category_mask').astype(bool).copy()
    cmask[:, -1] = True
    lens = hm.sum(axis=1)
    assert (lens == 0).any() and (lens == hm.shape[1]).any(), lens
    counts = np.stack([(cidx == c).sum(axis=1) for c in range(cmask.shape[1])], axis=1)
    assert (counts >= 2).any() and ((counts == 0) & cmask).any()
    st = _state(case)
    key = 'user_encoder.clusterFeatureAffine.bias' if 'wo_GCN' in tag else 'user_encoder.proxy_node_embedding'
    assert float(np.abs(st[key]).max()) > 1e-2
    mut = case.expect('mutated_user_history_category_mask')
    orig = case.expect('in/user_history_category_mask')
    if 'wo_GCN' in tag:                                   # the in-place write of variantEncoders.py:369 ...
        assert (mut[:, -1] == 1).all() and (orig[:, -1] == 0).any() and np.array_equal(mut[:, :-1], orig[:, :-1])
    else:                                                 # ... which SUE_wo_HCA does not make
        assert np.array_equal(mut, orig) and (orig[:, -1] == 0).any()
