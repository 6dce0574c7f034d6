"""Host tests of the news-encoder ablations CNE_Title / CNE_Content / CNE_wo_CS / CNE_wo_CA (variantEncoders.py:14-99,190-339): the public
surface, initialize(), the float64 restatement tests/cne_ablation_ref.py against the fixtures captured from the reference's own code and
against itself (permutations, the gate's partner), and what the fixtures must contain."""
import numpy as np
import pytest
import torch

import cne_ablation_ref as R
from golden_io import GoldenCase

NAMES = ['CNE_Title', 'CNE_Content', 'CNE_wo_CS', 'CNE_wo_CA']
TINY = ['tiny_CNE_Title_ATT', 'tiny_CNE_Content_ATT', 'tiny_CNE_wo_CS_ATT', 'tiny_CNE_wo_CS_SUE_stable', 'tiny_CNE_wo_CA_ATT_stable',
        'tiny_CNE_wo_CA_SUE_stable']
FULL = ['full_CNE_Title_ATT_g1p0', 'full_CNE_wo_CS_ATT_g1p0', 'full_CNE_wo_CA_ATT_g1p0_stable']
GPU_OUT_BAR = 2e-5          # TIGHT of tests/test_hip_cne_ablation_gpu.py


def _cfg(**over):
    from nnr_amd import config
    kw = dict(news_encoder='CNE_wo_CS', user_encoder='ATT', vocabulary_size=30, word_embedding_dim=8, hidden_dim=6, max_history_num=6, category_num=3,
              attention_dim=8, category_embedding_dim=5, subCategory_embedding_dim=7)
    kw.update(over)
    return config.make_config([], **kw)


def _model(cfg):
    from nnr_amd.model import Model
    return Model(cfg, torch.zeros(cfg.vocabulary_size, cfg.word_embedding_dim))


def _model_of(case):
    from nnr_amd.model import Model
    return Model(case.config, case.word_table())


def _state(case):
    return case.initial_state({k: tuple(p.shape) for k, p in _model_of(case).named_parameters()})


def _batch(case):
    from nnr_amd.synth import BATCH_FIELDS
    return {k: case.expect('in/' + k) for k in BATCH_FIELDS}


# ------------------------------------------------------------------------------------------------ flags and dispatch
def test_the_variant_list():
    from nnr_amd import config
    assert config.VARIANT_NEWS_ENCODERS == NAMES
    assert not set(config.VARIANT_NEWS_ENCODERS) & set(config.ALL_NEWS_ENCODERS)


@pytest.mark.parametrize('user', ['ATT', 'SUE'])
@pytest.mark.parametrize('name', NAMES)
def test_dispatch_and_flags(name, user):
    from nnr_amd import news_encoders, step
    cfg = _cfg(news_encoder=name, user_encoder=user)
    m = _model(cfg)
    ne = m.news_encoder
    assert type(ne) is getattr(news_encoders, name) and m.user_encoder.news_encoder is ne and m.model_name == name + '-' + user
    streams = 1 if name in ('CNE_Title', 'CNE_Content') else 2
    assert ne.news_embedding_dim == m.news_embedding_dim == 2 * cfg.hidden_dim * streams + 5 + 7
    assert ne.batch_independent is (name != 'CNE_wo_CA')
    assert ne.pad_dedup is False
    assert ne.max_title_length == cfg.max_title_length and ne.max_content_length == cfg.max_abstract_length
    assert hasattr(ne, 'forward_pair')
    assert step.kind(m.train()) is None
    for order in ('stable', 'torch'):                         # --tie_order is accepted by all four
        assert _model(_cfg(news_encoder=name, user_encoder=user, tie_order=order)).news_encoder.tie_order == order


@pytest.mark.parametrize('tag', TINY + FULL)
def test_parameter_names_are_the_fixtures(tag):
    case = GoldenCase(tag)
    m = _model_of(case)
    assert sorted(k for k, _ in m.named_parameters()) == sorted(case.param_names())
    assert type(m.news_encoder).__name__ == case.config.news_encoder
    if case.full_arrays:
        for k, p in m.named_parameters():
            assert tuple(p.shape) == tuple(case.expect('grad/' + k).shape), k
    lstm = [k for k in case.param_names() if '_lstm.' in k and k.startswith('news_encoder.')]
    stream = {'CNE_Title': ['title'], 'CNE_Content': ['content']}.get(case.config.news_encoder, ['title', 'content'])
    assert sorted(lstm) == sorted('news_encoder.%s_lstm.%s_l0%s' % (s, w, r) for s in stream for w in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')
                                  for r in ('', '_reverse'))


def test_both_refusals_keep_their_patterns_and_name_the_new_encoders():
    for over, old in ((dict(news_encoder='NAML'), 'NAML is not on the MI355X hot path .*HDC, PNE, DAE, Inception, KCNN, NAML_Title, NAML_Content'),
                      (dict(user_encoder='LSTUR'), 'LSTUR is not on the MI355X hot path .*CATT, FIM, OMAP, PUE, GRU'),
                      (dict(news_encoder='LSTUR'), r'is not on the MI355X hot path .*SUE_wo_GCN, SUE_wo_HCA\)$'),
                      (dict(user_encoder='LSTUR'), r'is not on the MI355X hot path .*SUE_wo_GCN, SUE_wo_HCA\)$')):
        with pytest.raises(Exception, match=old) as e:
            _model(_cfg(**over))
        assert 'CNE_Title, CNE_Content, CNE_wo_CS, CNE_wo_CA' in str(e.value)


# ------------------------------------------------------------------------------------------------ initialize()
@pytest.mark.parametrize('name', NAMES)
def test_initialize_is_the_references(name):
    torch.manual_seed(5)
    cfg = _cfg(news_encoder=name, hidden_dim=40, attention_dim=30, word_embedding_dim=24)
    m = _model(cfg)
    ne = m.news_encoder
    with torch.no_grad():
        for p in ne.parameters():
            p.fill_(7.0)
    m.initialize()
    streams = {'CNE_Title': ['title'], 'CNE_Content': ['content']}.get(name, ['title', 'content'])
    xavier = []
    for s in streams:
        lstm = getattr(ne, s + '_lstm')
        for k, q in lstm.named_parameters():
            q = q.detach().double()
            if q.dim() == 1:
                assert float(q.abs().max()) == 0.0, k
            else:                                             # orthogonal: the columns of the tall matrix are orthonormal
                assert float((q.t() @ q - torch.eye(q.shape[1], dtype=torch.float64)).abs().max()) <= 1e-5, k
        sa = getattr(ne, s + '_self_attention')
        assert float(sa.affine1.bias.detach().abs().max()) == 0.0
        xavier += [(sa.affine1.weight, 5.0 / 3), (sa.affine2.weight, 1.0)]
        if name == 'CNE_wo_CA':
            assert float(getattr(ne, s + '_M').bias.detach().abs().max()) == 0.0 and getattr(ne, s + '_H').bias is None
            xavier += [(getattr(ne, s + '_H').weight, 1.0), (getattr(ne, s + '_M').weight, 1.0)]
        if name == 'CNE_wo_CS':
            ca = getattr(ne, s + '_cross_attention')
            assert float(ca.Q.bias.detach().abs().max()) == 0.0 and ca.K.bias is None
            xavier += [(ca.K.weight, 1.0), (ca.Q.weight, 1.0)]
    for w, gain in xavier:
        w = w.detach()
        bound = gain * (6.0 / (w.shape[0] + w.shape[1])) ** 0.5
        assert 0.8 * bound <= float(w.abs().max()) <= bound * (1 + 1e-6)
    for t in (ne.category_embedding.weight, ne.subCategory_embedding.weight):      # the base class's own initialize()
        assert 0.05 <= float(t.detach().abs().max()) <= 0.1
    assert float(ne.subCategory_embedding.weight[0].detach().abs().max()) == 0.0
    gated, crossed = hasattr(ne, 'title_H') or hasattr(ne, 'content_H'), hasattr(ne, 'title_cross_attention')
    assert (gated, crossed) == (name == 'CNE_wo_CA', name == 'CNE_wo_CS')


# ------------------------------------------------------------------------------------------------ restatement against the fixtures
@pytest.mark.parametrize('tag', TINY + FULL)
def test_restatement_gives_the_fixtures_representations(tag):
    """cand_rep and hist_rep of the reference's own fp32 run against the float64 restatement."""
    case = GoldenCase(tag)
    got = R.encode_batch(case.config.news_encoder, _state(case), case.config, _batch(case))
    for k in ('cand_rep', 'hist_rep'):
        exp = torch.from_numpy(case.expect(k)).double()
        err = float((got[k] - exp).abs().max())
        print('%s: restatement vs the reference fp32 %s %.3e (max|.| %.3f)' % (tag, k, err, float(exp.abs().max())))
        assert err <= 2e-6, (k, err)


@pytest.mark.parametrize('tag', TINY)
def test_restatement_gradients_follow_the_references_float64_run(tag):
    case = GoldenCase(tag)
    douts = [case.expect('f64/dcand_rep'), case.expect('f64/dhist_rep')]
    got = R.encode_batch(case.config.news_encoder, _state(case), case.config, _batch(case), douts=douts)
    for k in ('cand_rep', 'hist_rep'):
        assert float((got[k] - torch.from_numpy(case.expect('f64/' + k))).abs().max()) <= 1e-12, k
    checked = 0
    for k, g in got.items():
        if k.startswith('grad/'):
            exp = torch.from_numpy(case.expect('f64/grad/news_encoder.' + k[5:]))
            assert float((g - exp).abs().max()) <= 1e-10 * max(1.0, float(exp.abs().max())), k
            checked += 1
    assert checked == len([k for k in case.param_names() if k.startswith('news_encoder.')])


# ------------------------------------------------------------------------------------------------ restatement properties
@pytest.mark.parametrize('tag', ['tiny_CNE_Title_ATT', 'tiny_CNE_Content_ATT', 'tiny_CNE_wo_CS_ATT'])
def test_permuting_the_news_of_a_call_permutes_the_representations(tag):
    case = GoldenCase(tag)
    b = _batch(case)
    base = R.encode_batch(case.config.news_encoder, _state(case), case.config, b)['hist_rep']
    B, Hn, D = base.shape
    perm = torch.randperm(B * Hn, generator=torch.Generator().manual_seed(3)).numpy()
    pb = dict(b)
    for k in ('title_text', 'title_mask', 'content_text', 'content_mask', 'category', 'subCategory'):
        v = b['user_' + k]
        pb['user_' + k] = v.reshape((B * Hn,) + v.shape[2:])[perm].reshape(v.shape)
    moved = R.encode_batch(case.config.news_encoder, _state(case), case.config, pb)['hist_rep']
    assert float((moved.reshape(B * Hn, D) - base.reshape(B * Hn, D)[perm]).abs().max()) <= 1e-12


@pytest.mark.parametrize('tag', ['tiny_CNE_wo_CA_ATT_stable', 'tiny_CNE_wo_CA_SUE_stable'])
def test_a_wrong_gate_partner_cannot_pass(tag):
    case = GoldenCase(tag)
    rank, index = (R.encode_batch('CNE_wo_CA', _state(case), case.config, _batch(case), pair=p)['hist_rep'] for p in ('rank', 'index'))
    move = float((rank - index).abs().max())
    print('%s: pairing by index instead of by sorted rank moves hist_rep by %.3e' % (tag, move))
    assert move >= 100 * GPU_OUT_BAR
    assert float((rank - torch.from_numpy(case.expect('hist_rep')).double()).abs().max()) <= 2e-6


# ------------------------------------------------------------------------------------------------ fixture conditions
@pytest.mark.parametrize('tag', TINY)
def test_tiny_fixtures_meet_their_conditions(tag):
    case = GoldenCase(tag)
    name = case.config.news_encoder
    assert int(case.meta['batch_size']) == 8 and int(case.meta['adam_steps']) == 3
    Lt, Lc = case.config.max_title_length, case.config.max_abstract_length
    tm = np.concatenate([case.expect('in/%s_title_mask' % c).reshape(-1, Lt) for c in ('news', 'user')]).astype(bool)
    cm = np.concatenate([case.expect('in/%s_content_mask' % c).reshape(-1, Lc) for c in ('news', 'user')]).astype(bool)
    assert (tm.sum(1) == 0).any(), 'no title with an all-zero mask'
    assert tm.all(axis=1).any(), 'no title of full length'
    assert (cm.sum(1) == 1).any(), 'no content of length 1'
    for key, L in (('in/user_title_mask', Lt), ('in/user_content_mask', Lc)):
        lens = case.expect(key).reshape(-1, L).astype(bool).sum(axis=1)
        _, counts = np.unique(lens[lens > 1], return_counts=True)
        assert (counts >= 2).any(), key
    hm = case.expect('in/user_history_mask').astype(bool)
    assert (~hm).any() and (case.expect('in/user_title_text')[~hm] == 0).all() and (case.expect('in/user_content_text')[~hm] == 0).all()
    # the in-place write reaches exactly the masks the variant reads
    reads = {'CNE_Title': ('title',), 'CNE_Content': ('content',)}.get(name, ('title', 'content'))
    for s in ('title', 'content'):
        acts = False                                          # CNE's write would change this stream's mask in at least one of the calls
        for call in ('news', 'user'):
            orig, mut = case.expect('in/%s_%s_mask' % (call, s)).astype(bool), case.expect('mutated_%s_%s_mask' % (call, s)).astype(bool)
            fixed = orig.copy()
            fixed[..., 0] = True
            acts = acts or not np.array_equal(fixed, orig)
            assert np.array_equal(mut, fixed if s in reads else orig), (call, s)
        assert acts, s
