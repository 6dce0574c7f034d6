"""CPU checks of the drop-in boundary: libnnr_hip.so loads and exports every symbol include/nnr_hip.h declares, and the
ctypes mirrors of the argument structs have the C layout.  No compute calls (there is no GPU in the build container)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nnr_hip.h')


def _declared():
    src = open(HEADER).read()
    return sorted(set(re.findall(r'^\s*(?:int|size_t)\s+(nnr_\w+)\s*\(', src, flags=re.M)))


def _params(name):
    """Parameter list of an entry point as declared in the header (comments stripped)."""
    src = re.sub(r'/\*.*?\*/', ' ', open(HEADER).read(), flags=re.S)
    m = re.search(r'\b(?:int|size_t)\s+%s\s*\(([^;{]*?)\)\s*;' % re.escape(name), src, flags=re.S)
    assert m, name
    body = ' '.join(m.group(1).split())
    return [] if body in ('', 'void') else [q.strip() for q in body.split(',')]


def _kind(param):
    """Kind (nnr_amd/_lib.py:SIGNATURES) that a parameter's C declaration maps to."""
    from nnr_amd import _lib
    if param.startswith('hipStream_t'):
        return 'stream'
    if '*' in param:
        base = param[:param.index('*')].replace('const', '').strip()
        if base in ('nnr_tape', 'nnr_dp_ctx'):
            return 'handle'
        if base == 'char':
            return 'cstr'
        return _lib.STRUCTS[base].__name__ if base in _lib.STRUCTS else 'ptr'
    ctype = param.rsplit(None, 1)[0].replace('const', '').strip()
    return {'int': 'i32', 'long': 'i64', 'int64_t': 'i64', 'size_t': 'u64', 'uint64_t': 'u64', 'float': 'f32', 'uint32_t': 'seed'}[ctype]


def test_library_exports_every_declared_symbol():
    """The .so exports every entry point of the header, and _lib.SIGNATURES -- from which the binding's argtypes / restype and the
    tape's encoding derive -- states exactly the header's entry points, each with the header's return type and parameter types."""
    from nnr_amd import _lib, tape
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    decl = _declared()
    assert len(decl) >= 30
    for name in decl:
        assert hasattr(lib, name), 'symbol %s declared in include/nnr_hip.h but not exported' % name
    assert sorted(_lib.SIGNATURES) == decl, 'nnr_amd/_lib.py:SIGNATURES must list exactly the header\'s entry points'
    assert _lib.SYMBOLS == list(_lib.SIGNATURES)
    src = open(HEADER).read()
    for name in decl:
        ret = re.search(r'^\s*(int|size_t)\s+%s\s*\(' % name, src, flags=re.M).group(1)
        assert _lib.SIGNATURES[name].split() == [{'int': 'i32', 'size_t': 'u64'}[ret]] + [_kind(q) for q in _params(name)], name
    name, index = tape.ADAM_STEP_ARG
    assert _params(name)[index].split()[-1] == 'step' and _lib.kinds(name)[index] == 'i32'
    bound = _lib.lib()
    for name in decl:
        assert len(getattr(bound, name).argtypes) == len(_params(name)), name
    assert bound.nnr_lstm_sync_bytes.restype is ctypes.c_size_t and bound.nnr_version.restype is ctypes.c_int
    assert lib.nnr_version() >= 1


def _c_fields(cls):
    return [('in' if f == 'inp' else f) for f, _ in cls._fields_]


def test_ctypes_structs_match_c_layout(tmp_path):
    """sizeof and every field's offsetof of every mirrored struct, against a C program generated from the mirrors' _fields_ (Python's
    `inp` is C's `in`)."""
    from nnr_amd import _lib
    exprs, want = [], []
    for cname, cls in sorted(_lib.STRUCTS.items()):
        exprs.append('sizeof(%s)' % cname)
        want.append(ctypes.sizeof(cls))
        for (pyname, _), cfield in zip(cls._fields_, _c_fields(cls)):
            exprs.append('offsetof(%s,%s)' % (cname, cfield))
            want.append(getattr(cls, pyname).offset)
    assert len(_lib.STRUCTS) == 6 and len(want) > 150
    src = tmp_path / 'sz.cpp'
    src.write_text('#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){size_t v[]={%s};'
                   'for(size_t i=0;i<sizeof(v)/sizeof(v[0]);i++)printf("%%zu\\n",v[i]);}\n' % (HEADER, ','.join(exprs)))
    exe = tmp_path / 'sz'
    subprocess.check_call(['hipcc', '-o', str(exe), str(src)], stderr=subprocess.DEVNULL)
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want, [e for e, g, w in zip(exprs, got, want) if g != w]


def test_tape_registry_matches_the_header():
    """csrc/tape.hip records and replays entry points through one generated thunk each (8-byte argument slots -> typed call):
    every entry point that takes a trailing hipStream_t must be recordable, with exactly the header's argument count; host-only
    queries must not be.  The pool struct's round-3 fields sit behind the round-2 ones (the Python mirror appends them)."""
    from nnr_amd import _lib
    lib = _lib.lib()
    n_rec = 0
    for name in _declared():
        ps = _params(name)
        fid = lib.nnr_tape_fn_id(name.encode())
        if ps and ps[-1].startswith('hipStream_t') and not name.startswith('nnr_tape_'):
            assert fid >= 0, '%s takes a stream but has no thunk in csrc/tape.hip REGISTRY' % name
            assert lib.nnr_tape_fn_nargs(fid) == len(ps) - 1, (name, lib.nnr_tape_fn_nargs(fid), ps)
            n_rec += 1
        else:
            assert fid < 0, '%s has no stream argument and must not be recordable' % name
    assert n_rec >= 50
    assert _lib.PoolArgs.th.offset > _lib.PoolArgs.lddv.offset and _lib.PoolArgs.w2.offset > _lib.PoolArgs.th.offset


def test_product_path_refuses_cpu_tensors():
    import torch
    from nnr_amd import ops, _lib
    with pytest.raises(_lib.NnrHipError):
        ops.add_(torch.zeros(8), torch.zeros(8))


def test_product_code_never_imports_the_oracle():
    pkg = os.path.join(ROOT, 'nnr_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                txt = open(os.path.join(dirpath, f)).read()
                assert 'oracle' not in txt.replace('oracle/nnr_oracle.py:length_order', ''), f + ' must not reference the oracle'
