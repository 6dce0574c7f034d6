"""Training wall time per epoch of nnr_amd.run.fit (profiles/run_summary.md): CNE+SUE at batch 64 on a synthetic corpus of the benchmark's
shape, N behaviours = N / 64 steps per epoch.  Compare ms_per_step with `python bench.py --gpus 1 --steps <N / 64> --warmup 5`.

    python tools/run_epoch_time.py [--behaviours 4096] [--epochs 4] [--root DIR]

An epoch's time runs from the end of the previous epoch's bookkeeping to the epoch-loss read-back: negative draw, order upload, every step's
batch gather and step, one synchronisation.  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from nnr_amd import run as R
    from nnr_amd.config import make_config
    from nnr_amd.model import Model
    ap = argparse.ArgumentParser()
    ap.add_argument('--behaviours', type=int, default=4096)
    ap.add_argument('--epochs', type=int, default=4)
    ap.add_argument('--batch_size', type=int, default=64)
    ap.add_argument('--root', default=None)
    a = ap.parse_args()
    cfg = make_config(['--news_encoder=CNE', '--user_encoder=SUE', '--dataset=small', '--epoch=%d' % a.epochs, '--batch_size=%d' % a.batch_size],
                      corpus_sizes=dict(user_num=a.behaviours))
    torch.manual_seed(0)
    device = torch.device('cuda', 0)
    train, dev_split, _ = R.synth_data(a.behaviours, cfg, device)
    model = Model(cfg)
    model.initialize()
    marks, paths = [], {}

    def log(msg):
        torch.cuda.synchronize()
        marks.append((time.perf_counter(), msg.split('\n')[0]))

    root = a.root or tempfile.mkdtemp(prefix='nnr_run_')
    res = R.fit(model.to(device), cfg, train, dev_split, R.RunDirs(root, cfg.dataset, model.model_name),
                on_step=lambda e, s, t: paths.setdefault(e, []).append(t.last_path), log=log)
    steps = -(-a.behaviours // a.batch_size)
    epochs = []
    for i, (t, m) in enumerate(marks):
        if m.endswith(': train done'):
            e = int(m.split()[1])
            ms = (t - marks[i - 1][0]) * 1000
            epochs.append(dict(epoch=e, train_ms=round(ms, 2), ms_per_step=round(ms / steps, 3), dev_ms=round((marks[i + 1][0] - t) * 1000, 2),
                               paths={p: paths[e].count(p) for p in sorted(set(paths[e]))}))
    print(json.dumps(dict(steps_per_epoch=steps, dev_samples=int(dev_split.corpus.num), epochs=epochs, losses=res.losses, best_epoch=res.best_epoch)))


if __name__ == '__main__':
    main()
