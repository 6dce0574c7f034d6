"""The pieces the evaluation paths share, the parts that need no GPU (nnr_amd.evaluate._distinct_rows / _split_like / eval_mode, the mode a
failed evaluation leaves behind, and the encoders' capability flags as their base classes declare them)."""
import inspect

import pytest
import torch


class Boom(Exception):
    pass


def _model(news='CNN', user='ATT'):
    from nnr_amd.config import make_config
    from nnr_amd.model import Model
    return Model(make_config(['--news_encoder=' + news, '--user_encoder=' + user], corpus_sizes=dict(vocabulary_size=50, user_num=7)))


def test_distinct_rows_reproduce_their_input():
    """6 rows, H = 3: rows 0 and 3 are equal, 1 and 4 differ in the mask only, 2 and 5 in the user only -> 5 distinct rows."""
    from nnr_amd.evaluate import _distinct_rows
    users = torch.tensor([4, 2, 6, 4, 2, 5], dtype=torch.int32)
    hist = torch.tensor([[7, 8, 0], [3, 1, 2], [9, 9, 1], [7, 8, 0], [3, 1, 2], [9, 9, 1]], dtype=torch.int32)
    hmask = torch.tensor([[1, 1, 0], [1, 1, 1], [1, 0, 0], [1, 1, 0], [1, 1, 0], [1, 0, 0]], dtype=torch.uint8)
    for mask in (hmask, hmask != 0):
        u, h, m, back = _distinct_rows(users, hist, mask)
        assert u.dtype == torch.int64 and h.dtype == torch.int64 and m.dtype == torch.bool and back.dtype == torch.int64
        assert tuple(u.shape) == (5,) and tuple(h.shape) == tuple(m.shape) == (5, 3) and tuple(back.shape) == (6,)
        assert torch.equal(u[back], users.long()) and torch.equal(h[back], hist.long()) and torch.equal(m[back], hmask != 0)
        assert back[0] == back[3] and len(set(back.tolist())) == 5
        key = torch.cat([u.view(-1, 1), h, m.long()], dim=1)
        assert len({tuple(r) for r in key.tolist()}) == 5                    # the returned rows are themselves distinct


def test_split_like_cuts_an_inverse_back_into_its_groups():
    from nnr_amd.evaluate import _split_like
    groups = (torch.tensor([[5, 3], [3, 9]]), torch.tensor([9, 1, 5]), torch.tensor([], dtype=torch.int64), torch.tensor([[1]]))
    used, inv = torch.unique(torch.cat([g.reshape(-1) for g in groups]), return_inverse=True)
    parts = _split_like(inv, groups)
    assert len(parts) == 4
    for g, p in zip(groups, parts):
        assert p.shape == g.shape and torch.equal(used[p], g)


@pytest.mark.parametrize('training', [True, False])
def test_eval_mode_restores_the_mode(training):
    from nnr_amd.evaluate import eval_mode
    net = torch.nn.Sequential(torch.nn.Linear(2, 2), torch.nn.Dropout(0.5)).train(training)
    with eval_mode(net) as inside:
        assert inside is net and not net.training and not net[1].training
    assert net.training is training and net[1].training is training
    with pytest.raises(Boom):
        with eval_mode(net):
            assert not net.training
            raise Boom()
    assert net.training is training and net[1].training is training


class _Corpus:
    """A split of 5 samples on the CPU that fails where a test wants it to."""
    num, H, device = 5, 3, torch.device('cpu')

    def __init__(self, t=None):
        self.t = t
        self.samples = torch.tensor([[1], [2], [3], [1], [2]], dtype=torch.int32)

    def train_batch(self, idx):
        raise Boom('train_batch')


class _NoNewsFields(dict):
    def __getitem__(self, k):
        if k.startswith('news_'):
            raise Boom(k)                                                   # the first thing encode_news_table reads
        return dict.__getitem__(self, k)


@pytest.mark.parametrize('training', [True, False])
def test_a_failed_evaluation_leaves_the_mode_it_found(training):
    from nnr_amd import evaluate as E
    model = _model().train(training)
    with pytest.raises(Boom, match='train_batch'):
        E.compute_scores(model, _Corpus(), 8, cache=False)
    assert model.training is training and model.news_encoder.training is training
    t = _NoNewsFields(beh_history=torch.tensor([[1, 2, 0]] * 5, dtype=torch.int32), beh_history_mask=torch.ones(5, 3, dtype=torch.bool),
                      beh_user=torch.zeros(5, dtype=torch.int32))
    for cache in (True, 'auto'):
        with pytest.raises(Boom, match='news_title_text'):
            E.compute_scores(model, _Corpus(t), 8, cache=cache)
        assert model.training is training and model.user_encoder.training is training


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('cache', ['auto', False])
def test_a_failed_dssm_evaluation_leaves_the_mode_it_found(cache, training):
    from nnr_amd import dssm

    class Towers(torch.nn.Module):
        feature_dim = 4

        def towers(self, *a):
            assert not self.training
            raise Boom('towers')

        def forward_ids(self, corpus, users, news):
            return self.towers(None, None)

    corpus = _Corpus()
    corpus.sample_user, corpus.sample_news = torch.tensor([0, 1, 1, 2, 0]), torch.tensor([3, 4, 3, 5, 5])
    corpus.user_ids = corpus.user_w = corpus.news_ids = corpus.news_w = None
    model = Towers().train(training)
    with pytest.raises(Boom, match='towers'):
        dssm.compute_scores(model, corpus, 2, cache=cache)
    assert model.training is training


NEWS_FLAGS = dict(batch_independent=False, cne_gate=False, pad_dedup=True, tie_order='stable')
USER_FLAGS = dict(needs_history_graph=False, needs_user_embedding=False, candidate_independent=False)


def _subclasses(module, base):
    return {n: c for n, c in inspect.getmembers(module, inspect.isclass) if issubclass(c, base) and c is not base and not n.startswith('_')}


def test_capability_flags_are_declared_once_with_the_defaults_the_reads_assumed():
    from nnr_amd import news_encoders as N, user_encoders as U
    for base, flags in ((N.NewsEncoder, NEWS_FLAGS), (U.UserEncoder, USER_FLAGS)):
        for name, default in flags.items():
            assert name in vars(base) and vars(base)[name] == default and type(vars(base)[name]) is type(default), (base.__name__, name)
    news, users = _subclasses(N, N.NewsEncoder), _subclasses(U, U.UserEncoder)
    assert set(news) == {'CNE', 'CNE_Title', 'CNE_Content', 'CNE_wo_CS', 'CNE_wo_CA', 'MHSA', 'CNN', 'PNE', 'NAML_Title', 'NAML_Content', 'DAE',
                         'Inception', 'KCNN', 'HDC'}
    assert set(users) == {'SUE', 'SUE_wo_GCN', 'SUE_wo_HCA', 'MHSA', 'ATT', 'GRU', 'CATT', 'OMAP', 'PUE', 'FIM'}

    def having(classes, flag, value=True):
        return {n for n, c in classes.items() if getattr(c, flag) == value}
    assert having(news, 'batch_independent') == {'CNE_Title', 'CNE_Content', 'CNE_wo_CS', 'MHSA', 'CNN', 'NAML_Title', 'NAML_Content', 'DAE',
                                                 'Inception', 'KCNN'}
    assert having(news, 'cne_gate') == {'CNE', 'CNE_wo_CA'}
    assert having(news, 'pad_dedup', False) == {'CNE_Title', 'CNE_Content', 'CNE_wo_CS', 'CNE_wo_CA'}
    assert having(news, 'tie_order', 'stable') == set(news)                  # the class default; the CNE family's instances follow --tie_order
    assert having(users, 'needs_history_graph') == {'SUE', 'SUE_wo_GCN', 'SUE_wo_HCA'}
    assert having(users, 'needs_user_embedding') == {'PUE'}
    assert having(users, 'candidate_independent') == {'ATT', 'MHSA', 'GRU', 'PUE', 'SUE_wo_HCA'}
    for classes in (news, users):                                            # every flag is a bool (or the tie order's name), never a None
        for c in classes.values():
            assert all(type(getattr(c, k)) is type(v) for k, v in {**NEWS_FLAGS, **USER_FLAGS}.items() if hasattr(c, k)), c.__name__


def test_the_flag_reads_carry_no_defaults_of_their_own():
    """evaluate.py and model.py read the flags as plain attributes: a per-site default would hide a misspelt flag on a new encoder."""
    import re
    from nnr_amd import evaluate, model
    names = '|'.join({**NEWS_FLAGS, **USER_FLAGS})
    for mod in (evaluate, model):
        assert not re.search(r'getattr\([^)]*[\'"](%s)[\'"]' % names, inspect.getsource(mod)), mod.__name__
