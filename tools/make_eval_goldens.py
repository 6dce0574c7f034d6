#!/usr/bin/env python3
"""Generate tests/golden/eval_*.npz by running the REFERENCE's own evaluation path -- util.compute_scores (util.py:10-68) and
evaluate.scoring (evaluate.py:32-89) -- with the reference's own model.py on the dev split of a tiny synthetic MIND tree.

Runs only in the build container.  Accommodations (none touches the arithmetic): the import stand-ins of tools/ref_shims,
a SimpleNamespace config, a temp CWD, `Tensor.cuda()` / `torch.cuda.empty_cache()` as no-ops (no GPU here: the reference
moves every batch to the GPU), and for the CNE fixture torch.sort forced stable (= the reference's pinned torch 1.12.1, see
tools/make_goldens.py).  The fixture holds arrays only: the dev corpus tables, the model's state_dict, and what the
reference produced: one score per (impression, candidate) sample, the per-impression ranks it wrote to the result file, the
labels of its truth file, and (AUC, MRR, nDCG@5, nDCG@10).
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference'
sys.path.insert(0, os.path.join(ROOT, 'tools', 'ref_shims'))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
OUT = os.path.join(ROOT, 'tests', 'golden')

from make_corpus_goldens import write_tree          # noqa: E402
from make_goldens import stable_sort_patch          # noqa: E402
from oracle.nnr_oracle import default_config        # noqa: E402  (attribute bag only)


def run(tag, news, user, stable, min_gap=None, batch_size=8, zero_ties=False, init_seed=5, **cfg_over):
    """`cfg_over`: flags default_config lacks (OMAP_head_num, HiFi_Ark_regularizer_coefficient: config.py:74-75; user_embedding_dim,
    personalized_embedding_dim: config.py:64-65).  `batch_size` is stored: PNE's scores depend on it (newsEncoders.py:359 pairs title row r
    of a batch with user r % batch).  `zero_ties`: impressions whose scores are ALL exactly zero (GRU: a user without history has a zero user
    vector) are left out of the gap check: their ties are exact on both sides, not rounding noise."""
    rng = np.random.default_rng(21)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        work = os.path.join(tmp, 'work')
        os.makedirs(work)
        write_tree(os.path.join(tmp, 'MIND-tiny'), rng)
        os.chdir(work)
        orig_cuda, orig_empty = torch.Tensor.cuda, torch.cuda.empty_cache
        torch.Tensor.cuda = lambda self, *a, **k: self
        torch.cuda.empty_cache = lambda: None
        try:
            import MIND_corpus, util, model as ref_model        # /root/reference
            flags = dict(news_encoder=news, user_encoder=user, dataset='tiny', word_threshold=1, max_title_length=8,
                         max_abstract_length=16, word_embedding_dim=16, hidden_dim=8, attention_dim=8, max_history_num=6,
                         category_embedding_dim=4, subCategory_embedding_dim=4, negative_sample_num=2, head_num=2, head_dim=4,
                         cnn_kernel_num=12, gcn_layer_num=2, dropout_rate=0.2, entity_embedding_dim=100, context_embedding_dim=100,
                         no_self_connection=False, no_adjacent_normalization=False, gcn_normalization_type='symmetric',
                         train_root='../MIND-tiny/train', dev_root='../MIND-tiny/dev', test_root='../MIND-tiny/test')
            flags.update(cfg_over)                              # (Inception overrides the two category dimensions)
            cfg = default_config(**flags)
            torch.manual_seed(init_seed)            # (initialize() draws from it; 5 unless a case needs another draw for its min_gap)
            corpus = MIND_corpus.MIND_Corpus(cfg)
            m = ref_model.Model(cfg)
            m.initialize()
            if user == 'GRU':
                m.user_encoder.device = torch.device('cpu')     # userEncoders.py:310,327: the empty users' zero rows go to self.device ('cuda')
                with torch.no_grad():                           # initialize() zeroes the biases: tanh(dec.bias) would hide the zero-row rule
                    gb = torch.Generator().manual_seed(77)
                    for k, p in m.user_encoder.named_parameters():
                        if not k.startswith('news_encoder.') and p.dim() == 1:
                            p.copy_(0.1 * torch.randn(p.shape, generator=gb))
            with torch.no_grad():                               # larger weights: scores spread out (ranks are then robust to fp32 noise)
                for k, p in m.named_parameters():
                    if 'word_embedding' not in k:
                        p.mul_(2.0)
            os.makedirs('dev/ref')
            os.makedirs('dev/res')
            with open(os.path.join(cfg.dev_root, 'behaviors.tsv'), encoding='utf-8') as dev_f, open('dev/ref/truth-tiny.txt', 'w', encoding='utf-8') as truth_f:
                for dev_ID, line in enumerate(dev_f):           # config.py:158-163
                    impressions = line.split('\t')[4]
                    labels = [int(i[-1]) for i in impressions.strip().split(' ')]
                    truth_f.write(('' if dev_ID == 0 else '\n') + str(dev_ID + 1) + ' ' + str(labels).replace(' ', ''))
            # capture the per-sample scores compute_scores keeps in a local: wrap the model's forward
            scores = []
            fwd = m.forward
            m.forward = lambda *a: (lambda o: (scores.append(o.detach().clone().numpy().reshape(-1)), o)[1])(fwd(*a))
            auc, mrr, ndcg5, ndcg10 = util.compute_scores(m, corpus, batch_size, 'dev', 'dev/res/out.txt', 'tiny')
            m.forward = fwd
            ranks, labels, sizes = [], [], []
            with open('dev/res/out.txt') as f:
                for line in f:
                    r = json.loads(line.strip().split()[1])
                    ranks += r
                    sizes.append(len(r))
            with open('dev/ref/truth-tiny.txt') as f:
                for line in f:
                    labels += json.loads(line.strip().split()[1])
            out = dict(scores=np.concatenate(scores).astype(np.float32), ranks=np.array(ranks, dtype=np.int32), labels=np.array(labels, dtype=np.uint8),
                       sizes=np.array(sizes, dtype=np.int32), metrics=np.array([auc, mrr, ndcg5, ndcg10], dtype=np.float64),
                       dev_indices=np.array(corpus.dev_indices, dtype=np.int32), batch_size=np.int64(batch_size),
                       category_num=np.int64(cfg.category_num), subCategory_num=np.int64(cfg.subCategory_num), vocabulary_size=np.int64(cfg.vocabulary_size),
                       user_num=np.int64(cfg.user_num), entity_size=np.int64(cfg.entity_size),
                       news_category=corpus.news_category, news_subCategory=corpus.news_subCategory, news_title_text=corpus.news_title_text,
                       news_title_mask=corpus.news_title_mask, news_title_entity=corpus.news_title_entity, news_abstract_text=corpus.news_abstract_text,
                       news_abstract_mask=corpus.news_abstract_mask, news_abstract_entity=corpus.news_abstract_entity,
                       beh_user=np.array([b[0] for b in corpus.dev_behaviors], dtype=np.int64),
                       beh_history=np.array([b[1] for b in corpus.dev_behaviors], dtype=np.int32),
                       beh_history_mask=np.array([b[2] for b in corpus.dev_behaviors], dtype=bool),
                       beh_candidate=np.array([b[3] for b in corpus.dev_behaviors], dtype=np.int32),
                       beh_line=np.array([b[4] for b in corpus.dev_behaviors], dtype=np.int32),
                       train_user_history_graph=corpus.dev_user_history_graph, train_user_history_category_mask=corpus.dev_user_history_category_mask,
                       train_user_history_category_indices=corpus.dev_user_history_category_indices)
            for k, v in m.state_dict().items():
                out['state/' + k] = v.numpy()
            cfgd = {k: v for k, v in vars(cfg).items() if isinstance(v, (int, float, str, bool))}
            out['cfg_keys'] = np.array(sorted(cfgd)).astype(str)
            out['cfg_vals'] = np.array([str(cfgd[k]) for k in sorted(cfgd)]).astype(str)
            out['cfg_types'] = np.array([type(cfgd[k]).__name__ for k in sorted(cfgd)]).astype(str)
            out['tie_order'] = np.array('stable' if stable else 'torch')
        finally:
            torch.Tensor.cuda, torch.cuda.empty_cache = orig_cuda, orig_empty
            os.chdir(cwd)
    if min_gap is not None:                             # the fixture must decide the ranks: no two scores of an impression closer than this
        o, gaps = 0, []
        for n in out['sizes']:
            if n > 1 and not (zero_ties and not out['scores'][o:o + n].any()):
                gaps.append(float(np.diff(np.sort(out['scores'][o:o + n])).min()))
            o += n
        assert min(gaps) > min_gap, (tag, min(gaps))
        print(tag, 'min within-impression score gap %.3e' % min(gaps))
    np.savez_compressed(os.path.join(OUT, 'eval_%s.npz' % tag), **out)
    print(tag, 'samples', out['scores'].shape[0], 'impressions', out['sizes'].shape[0], 'metrics', out['metrics'], 'score range', out['scores'].min(), out['scores'].max())


def run_metrics():
    """evaluate.py's own scoring() and per-impression functions on 300 ragged impressions (2..300 candidates, 1..many clicks)."""
    import io
    import evaluate                                          # /root/reference/evaluate.py
    rng = np.random.default_rng(33)
    sizes = np.concatenate([[2, 2, 3, 300, 299, 17], rng.integers(2, 120, size=294)]).astype(np.int32)
    labels, ranks, per = [], [], []
    truth, sub = io.StringIO(), io.StringIO()
    for i, n in enumerate(sizes):
        y = np.zeros(n, dtype=np.uint8)
        y[rng.choice(n, size=int(rng.integers(1, max(2, min(n - 1, 6)))), replace=False)] = 1
        r = (rng.permutation(n) + 1).astype(np.int32)
        labels.append(y); ranks.append(r)
        truth.write(('' if i == 0 else '\n') + str(i + 1) + ' ' + str(y.tolist()).replace(' ', ''))
        sub.write(('' if i == 0 else '\n') + str(i + 1) + ' ' + str(r.tolist()).replace(' ', ''))
        ys, sc = y.astype('float32'), [1. / v for v in r]
        per.append([evaluate.roc_auc_score(ys, sc), evaluate.mrr_score(ys, sc), evaluate.ndcg_score(ys, sc, 5), evaluate.ndcg_score(ys, sc, 10)])
    truth.seek(0); sub.seek(0)
    means = evaluate.scoring(truth, sub)
    np.savez_compressed(os.path.join(OUT, 'eval_metrics_ragged.npz'), sizes=sizes, labels=np.concatenate(labels), ranks=np.concatenate(ranks),
                        per_impression=np.array(per, dtype=np.float64), metrics=np.array(means, dtype=np.float64))
    print('metrics_ragged', len(sizes), 'impressions', int(sizes.sum()), 'samples', means)


def run_npa():
    """`python tools/make_eval_goldens.py npa`: PNE + PUE on the user-id embedding path, at batch size 8."""
    run('tiny_PNE_PUE', 'PNE', 'PUE', False, min_gap=1e-3, batch_size=8, user_embedding_dim=6, personalized_embedding_dim=10)


def run_bow():
    """`python tools/make_eval_goldens.py bow`: the two bag-of-words news encoders under ATT (Alpha: config.py:76; Inception needs the
    three embedding dimensions equal)."""
    run('tiny_DAE_ATT', 'DAE', 'ATT', False, min_gap=1e-4, Alpha=0.1)     # (sigmoid features: scores closer together than the others')
    run('tiny_Inception_ATT', 'Inception', 'ATT', False, min_gap=1e-3, category_embedding_dim=16, subCategory_embedding_dim=16)


def run_kcnn():
    """`python tools/make_eval_goldens.py kcnn`: the KCNN news encoder under CATT.  The tiny tree names an entity in every third title and
    holds both .vec files: the corpus writes the two knowledge pickles the reference's KCNN reads."""
    run('tiny_KCNN_CATT', 'KCNN', 'CATT', False, min_gap=1e-3)


def run_gru():
    """`python tools/make_eval_goldens.py gru`: DAE + GRU (random biases: see run())."""
    run('tiny_DAE_GRU', 'DAE', 'GRU', False, min_gap=1e-4, zero_ties=True, Alpha=0.1)


def run_naml():
    """`python tools/make_eval_goldens.py naml`: NAML_Title under ATT.  (The view softmax averages three rows: the scores lie closer together
    than the concatenating encoders'; the smallest gap inside an impression is 8.3e-5, forty times the fp32 error of a score.)"""
    run('tiny_NAML_Title_ATT', 'NAML_Title', 'ATT', False, min_gap=5e-5)


def run_fim():
    """`python tools/make_eval_goldens.py fim`: the HDC / FIM pair with its own click head, at the tiny FIM sizes of tools/make_goldens.py
    (history 11 so that both pooled layers keep a cell; S = 10 -> 8 -> 4 -> 2 -> 1)."""
    run('tiny_HDC_FIM', 'HDC', 'FIM', False, min_gap=1e-3, click_predictor='FIM', max_history_num=11, HDC_window_size=3, HDC_filter_num=6,
        conv3D_filter_num_first=3, conv3D_kernel_size_first=3, conv3D_filter_num_second=2, conv3D_kernel_size_second=3, maxpooling3D_size=2,
        maxpooling3D_stride=2)


def run_sue_ablation():
    """`python tools/make_eval_goldens.py sue_ablation`: the two user-encoder ablations of variantEncoders.py under CNN."""
    run('tiny_CNN_SUE_wo_GCN', 'CNN', 'SUE_wo_GCN', False, min_gap=1e-4)
    run('tiny_CNN_SUE_wo_HCA', 'CNN', 'SUE_wo_HCA', False, min_gap=1e-4)


def run_cne_ablation():
    """`python tools/make_eval_goldens.py cne_ablation`: two of the news-encoder ablations of variantEncoders.py under ATT -- CNE_wo_CS, whose
    representations depend on their own news only (the cached evaluation path), and CNE_wo_CA, whose gate pairs the news of a call by
    sorted rank (the per-sample path; torch.sort forced stable as for the CNE fixtures)."""
    run('tiny_CNE_wo_CS_ATT', 'CNE_wo_CS', 'ATT', False, min_gap=1e-4, init_seed=6)     # (seed 5: two scores of an impression 1.6e-5 apart)
    with stable_sort_patch():
        run('tiny_CNE_wo_CA_ATT_stable', 'CNE_wo_CA', 'ATT', True, min_gap=1e-4)


if __name__ == '__main__':
    torch.set_num_threads(4)
    if len(sys.argv) > 1 and sys.argv[1] == 'cne_ablation':
        run_cne_ablation()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == 'sue_ablation':
        run_sue_ablation()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == 'fim':
        run_fim()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == 'gru':
        run_gru()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == 'naml':
        run_naml()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == 'kcnn':
        run_kcnn()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == 'npa':
        run_npa()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == 'bow':
        run_bow()
        sys.exit(0)
    run_metrics()
    run('tiny_MHSA_MHSA', 'MHSA', 'MHSA', False)
    run('tiny_CNN_ATT', 'CNN', 'ATT', False)
    with stable_sort_patch():
        run('tiny_CNE_SUE_stable', 'CNE', 'SUE', True)
    run('tiny_CNN_CATT', 'CNN', 'CATT', False, min_gap=1e-3)
    with stable_sort_patch():
        run('tiny_CNE_CATT_stable', 'CNE', 'CATT', True, min_gap=1e-3)
    omap = dict(OMAP_head_num=3, HiFi_Ark_regularizer_coefficient=0.1)
    run('tiny_CNN_OMAP', 'CNN', 'OMAP', False, min_gap=1e-3, **omap)
    with stable_sort_patch():
        run('tiny_CNE_OMAP_stable', 'CNE', 'OMAP', True, min_gap=1e-3, **omap)
    run_npa()
    run_bow()
    run_kcnn()
    run_fim()
    run_gru()
    run_naml()
    run_sue_ablation()
    run_cne_ablation()
