#!/usr/bin/env python3
"""Per-epoch cost of negative sampling (profiles/negsample_summary.md): the reference's host loop (nnr_amd.corpus.negative_sampling over
numpy.random.randint, then the upload through DeviceCorpus.set_samples' copy) against the device sampler (nnr_negative_sample through
corpus.NegativeSampler.draw), on the same synthetic impression lists: `--behaviours` lists of 1..59 non-clicks, K = `--negatives`.

  python tools/negsample_bench.py [--behaviours 100000] [--negatives 4] [--epochs 2000]

The device figure is HIP events around `--epochs` consecutive draws (epoch 0 .. epochs - 1, after 3 warm-up draws), divided by their number;
the host figure is one timed pass of the loop plus its upload.  One JSON line on stdout (with the library's build id)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nnr_amd import _lib                                                        # noqa: E402
from nnr_amd.corpus import NegativeSampler, impression_lists, negative_sampling   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--behaviours', type=int, default=100000)
    ap.add_argument('--negatives', type=int, default=4)
    ap.add_argument('--epochs', type=int, default=2000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('negsample_bench needs a GPU: a timing taken elsewhere says nothing about the device sampler')
    torch.zeros(1, device='cuda')                                               # the first touch of the device is not the upload's cost
    torch.cuda.synchronize()
    rng = np.random.default_rng(0)
    beh = [(int(rng.integers(1, 65000)), rng.integers(1, 65000, size=int(n)).tolist()) for n in rng.integers(1, 60, size=a.behaviours)]
    np.random.seed(0)
    t0 = time.perf_counter()
    table = negative_sampling(beh, a.negatives, np.random.randint)
    host_loop = time.perf_counter() - t0
    t0 = time.perf_counter()
    up = torch.as_tensor(np.ascontiguousarray(table), dtype=torch.int32).to('cuda')
    torch.cuda.synchronize()
    host_upload = time.perf_counter() - t0
    sampler = NegativeSampler(*impression_lists(beh), 'cuda')
    for e in range(3):
        sampler.draw(e, 0, a.negatives)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for e in range(a.epochs):
        sampler.draw(e, 0, a.negatives)
    end.record()
    torch.cuda.synchronize()
    device_us = start.elapsed_time(end) * 1e3 / a.epochs
    lists_bytes = sum(t.numel() * t.element_size() for t in (sampler.clicks, sampler.neg_offsets, sampler.neg_ids))
    print(json.dumps({'tool': 'negsample_bench', 'behaviours': a.behaviours, 'negatives': a.negatives, 'non_clicks': int(sampler.neg_ids.numel()),
                      'host_loop_s': round(host_loop, 3), 'host_upload_ms': round(host_upload * 1e3, 3), 'device_us_per_epoch': round(device_us, 2),
                      'device_epochs_timed': a.epochs, 'lists_resident_bytes': lists_bytes, 'table_bytes': int(up.numel() * 4),
                      'device': torch.cuda.get_device_name(0), 'build': _lib.build_id()}))


if __name__ == '__main__':
    main()
