"""The seven weight layouts of nnr_amd.ops.LAYOUTS restated with torch.permute / flip, for the host test of the table
(tests/test_weight_layouts.py) and the GPU test of nnr_permute (tests/test_hip_kcnn_gpu.py)."""
import torch

KCNN_DIMS = [(12, 16, 3), (5, 10, 4), (3, 7, 1)]                 # (C, E, w): KCNN's Conv2d weight, J = 3
C1_DIMS = [(12, 16, 3, 1), (5, 10, 5, 1), (3, 7, 1, 1), (4, 6, 7, 1)]      # (C, E, k, J = 1): the Conv1d weight in the same kinds
HDC_DIMS = [(6, 10, 3, 10), (5, 7, 3, 8), (1, 1, 1, 1)]          # (F, C, w, ldp)
C3_DIMS = [(5, 4, 3), (3, 5, 2), (4, 4, 1)]                      # (Cout, Cin, K)
CASES = ([(k, d) for k in ('kcnn_p', 'kcnn_q', 'kcnn_dw') for d in KCNN_DIMS + C1_DIMS] + [(k, d) for k in ('hdc_p', 'hdc_dw') for d in HDC_DIMS] +
         [(k, d) for k in ('c3_p', 'c3_q') for d in C3_DIMS])


def source_shape(kind, dims):
    if kind.startswith('kcnn'):
        C, E, w, J = dims if len(dims) == 4 else dims + (3,)
        return (C, w, J, E) if kind == 'kcnn_dw' else (C, E, w, J)
    if kind.startswith('hdc'):
        F, C, w, ldp = dims
        return (w, F, ldp) if kind == 'hdc_dw' else (F, C, w)
    Cout, Cin, K = dims
    return (Cout, Cin, K ** 3)


def source(kind, dims, seed=0):
    return torch.randn(source_shape(kind, dims), generator=torch.Generator().manual_seed(seed + sum(dims)))


def expected(kind, src, dims, into):
    """`into` (the destination before the call, in the table's destination shape) with the written elements replaced; the rest keeps its bits."""
    out = into.clone()
    if kind == 'kcnn_p':
        out.view(src.shape[0], src.shape[2], src.shape[3], src.shape[1])[:] = src.permute(0, 2, 3, 1)
    elif kind == 'kcnn_q':
        out.view(src.shape[3], src.shape[1], src.shape[2], src.shape[0])[:] = src.flip(2).permute(3, 1, 2, 0)
    elif kind == 'kcnn_dw':
        out[:] = src.permute(0, 3, 1, 2)
    elif kind == 'hdc_p':
        out[:, :, :dims[1]] = src.permute(2, 0, 1)
    elif kind == 'hdc_dw':
        out[:] = src[:, :, :dims[1]].permute(1, 2, 0)
    elif kind == 'c3_p':
        out[:, :, :dims[0]] = src.permute(1, 2, 0)
    elif kind == 'c3_q':
        out[:, :, :dims[1]] = src.permute(0, 2, 1)
    else:
        raise KeyError(kind)
    return out
