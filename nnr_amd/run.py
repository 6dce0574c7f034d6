"""The training run: the reference's Trainer.train (trainer.py:74-196) and main.py's train / dev / test modes over
the pieces this package already has -- DeviceCorpus.sample_negatives / train_batch, Trainer.train_step, evaluate.evaluate -- plus the
bookkeeping around them: model selection by --dev_criterion, early stopping, checkpoints, rank files and result files in the reference's
directory layout.  Single process; the data-parallel run loop (distributed_train) is not here.

No kernel of its own: inside an epoch the driver slices one uploaded index tensor, calls train_batch / train_step and adds loss * B to a
float64 device scalar.  It adds no host synchronisation and no host-to-device copy to a step; the epoch loss is read once, after the last step.

    python -m nnr_amd.run --news_encoder=CNE --user_encoder=SUE --data DIR        (train.npz / dev.npz / test.npz)
    python -m nnr_amd.run --news_encoder=CNN --user_encoder=ATT --synth 4096      (a synthetic corpus from nnr_amd.synth)

Imports on a machine without a GPU (as nnr_amd.evaluate does); everything that launches needs one."""
import json
import os
import shutil
import zipfile

import numpy as np
import torch

from . import dp
from . import evaluate as E

CRITERIA = ('auc', 'mrr', 'ndcg5', 'ndcg10', 'avg')


class AvgMetric:
    """util.py:83-104: the four dev metrics ordered by avg = (auc + mrr + (ndcg5 + ndcg10) / 2) / 3."""

    def __init__(self, auc, mrr, ndcg5, ndcg10):
        self.auc, self.mrr, self.ndcg5, self.ndcg10 = auc, mrr, ndcg5, ndcg10
        self.avg = (auc + mrr + (ndcg5 + ndcg10) / 2) / 3

    def __gt__(self, other):
        return self.avg > other.avg

    def __ge__(self, other):
        return self.avg >= other.avg

    def __lt__(self, other):
        return self.avg < other.avg

    def __le__(self, other):
        return self.avg <= other.avg

    def __str__(self):
        return '%.4f\nAUC = %.4f\nMRR = %.4f\nnDCG@5 = %.4f\nnDCG@10 = %.4f' % (self.avg, self.auc, self.mrr, self.ndcg5, self.ndcg10)


class Selection:
    """Model selection and early stopping of trainer.py:132-185, single-process form.  An epoch improves when its criterion is >= the best
    so far (the best starts at 0, at AvgMetric(0, 0, 0, 0) for 'avg'), so a tie moves best_epoch to the later epoch and resets the counter.
    `stop` is epoch_not_increase == early_stopping_epoch (trainer.py:184); the distributed loop's `>` (trainer.py:374), which runs one epoch
    longer, is not followed."""

    def __init__(self, criterion='avg', early_stopping_epoch=5):
        if criterion not in CRITERIA:
            raise ValueError('dev_criterion=%r (one of %s)' % (criterion, ', '.join(CRITERIA)))
        self.criterion, self.early_stopping_epoch = criterion, int(early_stopping_epoch)
        self.best = AvgMetric(0, 0, 0, 0) if criterion == 'avg' else 0
        self.best_epoch = 0
        self.epoch_not_increase = 0

    def update(self, epoch, auc, mrr, ndcg5, ndcg10):
        """Account for `epoch`'s dev metrics; True when it is the best epoch so far (ties included)."""
        value = AvgMetric(auc, mrr, ndcg5, ndcg10) if self.criterion == 'avg' else dict(auc=auc, mrr=mrr, ndcg5=ndcg5, ndcg10=ndcg10)[self.criterion]
        improved = bool(value >= self.best)
        if improved:
            self.best, self.best_epoch, self.epoch_not_increase = value, epoch, 0
        else:
            self.epoch_not_increase += 1
        return improved

    @property
    def stop(self):
        return self.epoch_not_increase == self.early_stopping_epoch


def get_run_index(result_dir):
    """util.py:71-80: one more than the largest k of the '#k-dev' files in `result_dir`; leaves the empty '#<index>-dev' behind, which
    reserves the index for this run."""
    top = 0
    for name in os.listdir(result_dir):
        name = name.strip()
        if name[:1] == '#' and name[-4:] == '-dev':
            top = max(top, int(name[1:-4]))
    with open(os.path.join(result_dir, '#%d-dev' % (top + 1)), 'w', encoding='utf-8'):
        pass
    return top + 1


class RunDirs:
    """The reference's directory layout (config.py:142-149) under `root`, where the reference uses the working directory: config_dir,
    model_dir, best_model_dir, dev_res_dir, test_res_dir, result_dir = <kind>/<dataset>/<model_name>, and prediction_dir (config.py:174) for
    a split without labels.  Reading one of these attributes creates the directory; path(name) does not."""
    LAYOUT = dict(config_dir='configs', model_dir='models', best_model_dir='best_model', dev_res_dir='dev/res', test_res_dir='test/res',
                  result_dir='results', prediction_dir='prediction')

    def __init__(self, root, dataset, model_name):
        self.root, self.dataset, self.model_name = str(root), str(dataset), str(model_name)

    def path(self, name):
        # (normpath: under root '.' the paths are the reference's own, 'best_model/...': a model path names its result directory, main.py:42)
        return os.path.normpath(os.path.join(self.root, *self.LAYOUT[name].split('/'), self.dataset, self.model_name))

    def __getattr__(self, name):
        if name not in RunDirs.LAYOUT:
            raise AttributeError(name)
        p = self.path(name)
        os.makedirs(p, exist_ok=True)
        return p

    def run_dir(self, name, run_index):
        """<dir>/#<run>, created (trainer.py:32-41)."""
        p = os.path.join(getattr(self, name), '#%d' % run_index)
        os.makedirs(p, exist_ok=True)
        return p


class Split:
    """A dev or test split: `corpus` a DeviceCorpus from evaluate.dev_corpus, `sizes` candidates per impression (file order), `labels` one
    per sample or None (MIND-large's test split)."""

    def __init__(self, corpus, sizes, labels=None):
        self.corpus = corpus
        self.sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
        self.labels = None if labels is None else np.asarray(labels).reshape(-1)


class RunResult:
    """What fit() did: run_index, best_epoch, epochs_run, per-epoch losses [float] and metrics [(auc, mrr, ndcg5, ndcg10)], best_model_path."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


# ------------------------------------------------------------------------------------------------ checkpoints
def checkpoint_state(model):
    """model.state_dict() as contiguous CPU tensors that own their storage (a parameter of a trained model is a view of the flat buffer:
    saved as it is, every entry would drag the whole buffer into the file).  The user_encoder.news_encoder.* aliases stay in, as in the
    reference's file, and share their copy with the news encoder's entry, so the file holds each tensor once."""
    state, copies = {}, {}
    for k, v in model.state_dict().items():
        key = (v.data_ptr(), tuple(v.shape), tuple(v.stride()), v.dtype)
        if key not in copies:
            copies[key] = v.detach().to('cpu', copy=True).contiguous()
        state[k] = copies[key]
    return state


def save_checkpoint(model, path):
    """The reference's checkpoint (trainer.py:183): torch.save({model_name: state_dict}); loads with weights_only=True and without this package."""
    torch.save({model.model_name: checkpoint_state(model)}, path)


def load_checkpoint(model, path, what):
    """main.py:39-40 / :53-54: `what` is 'Dev' or 'Test'."""
    if not os.path.exists(path):
        raise AssertionError('%s model does not exist : %s' % (what, path))
    model.load_state_dict(torch.load(path, map_location='cpu', weights_only=True)[model.model_name], strict=True)


# ------------------------------------------------------------------------------------------------ result files
def result_line(tag, auc, mrr, ndcg5, ndcg10):
    """'#<tag>\\t<auc>\\t<mrr>\\t<ndcg5>\\t<ndcg10>\\n' with str(float) numbers (trainer.py:137, main.py:66,69)."""
    return '#' + str(tag) + '\t' + str(auc) + '\t' + str(mrr) + '\t' + str(ndcg5) + '\t' + str(ndcg10) + '\n'


def dev_log_text(metrics):
    """trainer.py:187-190: one line per epoch run."""
    return 'Epoch\tAUC\tMRR\tnDCG@5\tnDCG@10\n' + ''.join('%d\t%.4f\t%.4f\t%.4f\t%.4f\n' % ((i + 1,) + tuple(m)) for i, m in enumerate(metrics))


def _write(path, text):
    with open(path, 'w', encoding='utf-8') as f:
        f.write(text)


def _flag_values(config):
    return {k: v for k, v in vars(config).items() if isinstance(v, (bool, int, float, str))}


def _refuse(config, train=None):
    """What the run loop does not cover, before anything is written."""
    if int(getattr(config, 'world_size', 1)) > 1 or dp.world_size() > 1:
        raise NotImplementedError('nnr_amd.run is the single-process loop (trainer.py:74-196): world_size=%d, process group of %d; the '
                                  'data-parallel run loop (distributed_train) is a later change' % (int(getattr(config, 'world_size', 1)), dp.world_size()))
    if train is not None:
        if int(config.epoch) < 1:
            raise ValueError('epoch=%d: a run trains at least one epoch (its best model is the test model)' % int(config.epoch))
        if getattr(train, 'sampler', None) is None:
            raise ValueError('the training corpus has no impression lists: call set_impressions() first (every epoch redraws its negatives '
                             'with sample_negatives)')


# ------------------------------------------------------------------------------------------------ train
def fit(model, config, train, dev, dirs, run_index=None, trainer=None, listwise=False, on_step=None, log=print, dedup=False):
    """Trainer.train (trainer.py:74-196) on the device.  `train`: a DeviceCorpus with impression lists (set_impressions); `dev`: a Split with
    labels; `dirs`: RunDirs.  Per epoch e = 1 .. config.epoch: redraw the negatives in place (sample_negatives(e)), visit the behaviours in
    dp.sampler_indices(n, 0, 1, e) order in batches of config.batch_size (the last one short), evaluate the dev split at batch_size * 3 // 2,
    write its rank file, and on improvement (Selection) the '#<run>-dev' line and the epoch's checkpoint; leave on Selection.stop.  Afterwards
    the dev log, the best model's copy and the flag values.  on_step(e, step, trainer) is called after every step (steps count from 1).
    listwise / dedup: evaluate()'s keywords (the opt-in evaluation forms; a model neither applies to keeps its path).
    -> RunResult."""
    _refuse(config, train)
    from .trainer import Trainer
    name, dev_of = model.model_name, train.device
    run = get_run_index(dirs.result_dir) if run_index is None else int(run_index)
    if trainer is None:
        trainer = Trainer(model, config)
    seed, K, B, n = int(getattr(config, 'seed', 0)), int(config.negative_sample_num), int(config.batch_size), int(train.num)
    sel = Selection(getattr(config, 'dev_criterion', 'avg'), getattr(config, 'early_stopping_epoch', 5))
    model_dir, res_dir = dirs.run_dir('model_dir', run), dirs.run_dir('dev_res_dir', run)
    total = torch.zeros((), device=dev_of, dtype=torch.float64)
    losses, metrics = [], []
    log('Running : %s\t#%d' % (name, run))
    for e in range(1, int(config.epoch) + 1):
        train.sample_negatives(e, seed=seed, negative_sample_num=K)
        order = dp.sampler_indices(n, 0, 1, e, seed=seed).to(dev_of)           # the epoch's one upload; a step's indices are a view of it
        model.train()
        total.zero_()
        for step, start in enumerate(range(0, n, B), 1):
            idx = order[start:start + B]
            _, loss = trainer.train_step(train.train_batch(idx))
            total += loss.reshape(()).double() * idx.numel()                    # float(loss) * user_ID.size(0) of trainer.py:115, left on the device
            if on_step is not None:
                on_step(e, step, trainer)
        losses.append(float(total) / n)                                         # the epoch's one read-back (trainer.py:122)
        log('Epoch %d : train done\nloss = %s' % (e, losses[-1]))
        m, ranks = E.evaluate(model, dev.corpus, dev.labels, dev.sizes, B * 3 // 2, listwise=listwise, dedup=dedup)
        E.write_result_file(os.path.join(res_dir, '%s-%d.txt' % (name, e)), ranks, dev.sizes.tolist())
        metrics.append(m)
        log('Epoch %d : dev done\nDev criterions\nAUC = %.4f\nMRR = %.4f\nnDCG@5 = %.4f\nnDCG@10 = %.4f' % ((e,) + m))
        if sel.update(e, *m):
            _write(os.path.join(dirs.result_dir, '#%d-dev' % run), result_line(run, *m))
            save_checkpoint(model, os.path.join(model_dir, '%s-%d' % (name, e)))
        log('Best epoch : %d\nBest %s : %s' % (sel.best_epoch, sel.criterion, sel.best))
        if sel.stop:
            break
    _write(os.path.join(res_dir, '%s-%s-dev_log.txt' % (name, dirs.dataset)), dev_log_text(metrics))
    if sel.best_epoch == 0:
        raise RuntimeError('no epoch reached a dev %s >= 0 (metrics: %r): there is no best model' % (sel.criterion, metrics))
    best = os.path.join(dirs.run_dir('best_model_dir', run), name)
    shutil.copy(os.path.join(model_dir, '%s-%d' % (name, sel.best_epoch)), best)
    with open(os.path.join(dirs.config_dir, '#%d.json' % run), 'w', encoding='utf-8') as f:
        json.dump(_flag_values(config), f)
    log('Training : %s #%d completed\nDev criterions:\nAUC : %.4f\nMRR : %.4f\nnDCG@5 : %.4f\nnDCG@10 : %.4f' % ((name, run) + metrics[sel.best_epoch - 1]))
    return RunResult(run_index=run, best_epoch=sel.best_epoch, epochs_run=len(losses), losses=losses, metrics=metrics, best_model_path=best)


# ------------------------------------------------------------------------------------------------ dev / test
def _score_split(model, config, split, res_root, model_path):
    """Load-independent part of main.py:42-45 / :56-61: evaluate at batch_size * 2 // world_size and write the rank file under
    <res_root>/<model path with its separators replaced by '_'>/<model_name>.txt.  -> (metrics or None, rank file)."""
    res_dir = os.path.join(res_root, model_path.replace('\\', '_').replace('/', '_'))
    os.makedirs(res_dir, exist_ok=True)
    batch = int(config.batch_size) * 2 // int(getattr(config, 'world_size', 1))
    model.to(split.corpus.device)
    if split.labels is not None:
        metrics, ranks = E.evaluate(model, split.corpus, split.labels, split.sizes, batch)
    else:                                                    # no truth file (util.py:63-68): ranks only
        scores = E.compute_scores(model, split.corpus, batch)
        ranks, metrics = E.rank_metrics(scores, torch.zeros(scores.numel(), dtype=torch.uint8), split.sizes)[0], None
    out = os.path.join(res_dir, model.model_name + '.txt')
    E.write_result_file(out, ranks, split.sizes.tolist())
    return metrics, out


def dev(model, config, split, dirs, log=print):
    """main.py:37-48: load config.dev_model_path into `model` (strict), score the dev split.  -> (auc, mrr, ndcg5, ndcg10)."""
    _refuse(config)
    path = getattr(config, 'dev_model_path', '')
    load_checkpoint(model, path, 'Dev')
    metrics, _ = _score_split(model, config, split, dirs.dev_res_dir, path)
    log('Dev : %s\nAUC : %.4f\nMRR : %.4f\nnDCG@5 : %.4f\nnDCG@10 : %.4f' % ((path,) + metrics))
    return metrics


def test(model, config, split, dirs, run_index=None, log=print):
    """main.py:51-75: load config.test_model_path into `model` (strict), score the test split.  With labels: the '#<run>-test' line in train
    mode, the '#<seed + 1>' line in --test_output_file in test mode.  Without (MIND-large): ranks only, None metrics, and in train mode
    prediction.txt + prediction.zip under <prediction_dir>/#<run>.  run_index defaults to config.run_index (main.py:30)."""
    _refuse(config)
    path, mode = getattr(config, 'test_model_path', ''), getattr(config, 'mode', 'train')
    run = getattr(config, 'run_index', None) if run_index is None else run_index
    if mode == 'train' and run is None:
        raise ValueError('test() in train mode files its result under the run index: pass run_index (or set config.run_index)')
    load_checkpoint(model, path, 'Test')
    log('test model path  : ' + path)
    metrics, out = _score_split(model, config, split, dirs.test_res_dir, path)
    log('test output file : ' + out)
    if metrics is not None:
        log('AUC : %.4f\nMRR : %.4f\nnDCG@5 : %.4f\nnDCG@10 : %.4f' % metrics)
        if mode == 'train':
            _write(os.path.join(dirs.result_dir, '#%d-test' % int(run)), result_line(int(run), *metrics))
        elif mode == 'test' and getattr(config, 'test_output_file', '') != '':
            _write(config.test_output_file, result_line(int(getattr(config, 'seed', 0)) + 1, *metrics))
    elif mode == 'train':
        pred = dirs.run_dir('prediction_dir', int(run))
        shutil.copy(out, os.path.join(pred, 'prediction.txt'))
        with zipfile.ZipFile(os.path.join(pred, 'prediction.zip'), 'w', zipfile.ZIP_DEFLATED) as z:
            z.write(os.path.join(pred, 'prediction.txt'), 'prediction.txt')
    return metrics


# ------------------------------------------------------------------------------------------------ command line
_SIZE_KEYS = ('vocabulary_size', 'category_num', 'subCategory_num', 'user_num', 'entity_size')


def _npz(data_dir, name):
    p = os.path.join(data_dir, name + '.npz')
    return np.load(p) if os.path.exists(p) else None


def _data_meta(data_dir):
    """corpus_sizes (the five values MIND_Corpus.__init__ injects) and the optional word_table: from the first split file that holds them."""
    sizes, table = {}, None
    for name in ('train', 'dev', 'test'):
        z = _npz(data_dir, name)
        if z is None:
            continue
        for k in _SIZE_KEYS:
            if k in z.files:
                sizes.setdefault(k, int(z[k]))
        if table is None and 'word_table' in z.files and z['word_table'].size:
            table = torch.from_numpy(np.ascontiguousarray(z['word_table'], dtype=np.float32))
    return sizes, table


def _load_train(data_dir, config, device):
    from .corpus import DeviceCorpus
    z = _npz(data_dir, 'train')
    if z is None:
        raise FileNotFoundError(os.path.join(data_dir, 'train.npz'))
    dc = DeviceCorpus({k: z[k] for k in z.files}, device, config.category_num, config=config)
    dc.set_impressions(z['clicks'], z['neg_offsets'], z['neg_ids'])
    return dc


def _load_split(data_dir, name, config, device, required=True):
    from .corpus import norm_from_config
    z = _npz(data_dir, name)
    if z is None:
        if required:
            raise FileNotFoundError(os.path.join(data_dir, name + '.npz'))
        return None
    dc = E.dev_corpus({k: z[k] for k in z.files}, device, config.category_num, norm=norm_from_config(config))
    return Split(dc, z['sizes'], z['labels'] if 'labels' in z.files else None)


def synth_data(n, config, device):
    """A synthetic corpus of `n` training behaviours over nnr_amd.synth's news pool, with dev and test splits of n // 8 impressions."""
    from .corpus import from_synth, from_synth_lists
    from .synth import SynthCorpus, SynthSpec
    spec = SynthSpec(vocabulary_size=config.vocabulary_size, category_num=config.category_num, subCategory_num=config.subCategory_num,
                     max_title_length=config.max_title_length, max_abstract_length=config.max_abstract_length,
                     max_history_num=config.max_history_num, negative_sample_num=config.negative_sample_num, seed=int(config.seed) + 1)
    synth, rng = SynthCorpus(spec), np.random.default_rng(int(config.seed) + 2)
    train = from_synth(synth, n, rng, device)
    lens = rng.integers(1, 4 * config.negative_sample_num, size=n)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    train.set_impressions(rng.integers(1, spec.news_pool, size=n), offsets, rng.integers(1, spec.news_pool, size=int(offsets[-1])))
    splits = []
    for _ in range(2):
        sizes = rng.integers(2, 21, size=max(4, n // 8))
        labels = np.concatenate([rng.permutation(s) < rng.integers(1, s) for s in sizes]).astype(np.uint8)     # >= 1 click, >= 1 non-click each
        splits.append(Split(from_synth_lists(synth, sizes, rng, device), sizes, labels))
    return train, splits[0], splits[1]


def main(argv=None):
    """python -m nnr_amd.run: the reference's flags (nnr_amd.config) plus --data DIR | --synth N.  The run directories go under the working
    directory, as the reference's do.  Mode dispatch of main.py:78-88: train = fit, then test on the best model; dev; test."""
    import argparse
    from .config import make_config
    from .model import Model
    p = argparse.ArgumentParser(add_help=False)
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument('--data', type=str)
    src.add_argument('--synth', type=int)
    own, rest = p.parse_known_args(argv)
    sizes, table = _data_meta(own.data) if own.data else (dict(user_num=max(1, own.synth)), None)     # (synthetic behaviours: one user each)
    config = make_config(rest, corpus_sizes=sizes)
    _refuse(config)
    if not torch.cuda.is_available():
        raise RuntimeError('nnr_amd.run needs a GPU: the corpus, the step and the evaluation live in libnnr_hip.so (no CPU path)')
    device = torch.device('cuda', int(config.device_id))
    torch.cuda.set_device(device)
    torch.manual_seed(int(config.seed))
    new_model = lambda: Model(config, table)
    dirs = RunDirs('.', config.dataset, config.news_encoder + '-' + config.user_encoder)
    if own.synth:
        train, dev_split, test_split = synth_data(own.synth, config, device)
    else:
        train = _load_train(own.data, config, device) if config.mode == 'train' else None
        dev_split = _load_split(own.data, 'dev', config, device) if config.mode in ('train', 'dev') else None
        test_split = _load_split(own.data, 'test', config, device, required=config.mode == 'test') if config.mode in ('train', 'test') else None
    if config.mode == 'train':
        model = new_model()
        model.initialize()
        result = fit(model.to(device), config, train, dev_split, dirs)
        if test_split is not None:
            config.run_index, config.test_model_path = result.run_index, result.best_model_path
            test(new_model(), config, test_split, dirs)
        return result
    if config.mode == 'dev':
        return dev(new_model(), config, dev_split, dirs)
    return test(new_model(), config, test_split, dirs)


if __name__ == '__main__':
    main()
