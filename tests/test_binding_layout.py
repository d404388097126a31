"""The binding's mirrors of include/hvo.h, checked against the header itself: a small program generated from the binding's record table
(RECORDS: C type name -> ctypes Structure or numpy dtype) prints sizeof and every field's offsetof and size as the host compiler sees
them, and the test compares them with what ctypes and numpy lay out.  CPU only."""
import ctypes
import importlib
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, PKG_DIR

COMPILERS = (["c++"], ["cc", "-x", "c++"], ["hipcc", "-x", "c++"])


def _fields(mirror):
    """(name, offset, size) of every field of a ctypes Structure or a structured dtype"""
    if isinstance(mirror, np.dtype):
        return [(k, mirror.fields[k][1], mirror.fields[k][0].itemsize) for k in mirror.names]
    return [(k, getattr(mirror, k).offset, getattr(mirror, k).size) for k, *_ in mirror._fields_]


def _sizeof(mirror):
    return mirror.itemsize if isinstance(mirror, np.dtype) else ctypes.sizeof(mirror)


@pytest.fixture(scope="module")
def header_layout(hvo, tmp_path_factory):
    """{C type: (sizeof, {field: (offsetof, size)})} as the host compiler lays include/hvo.h out"""
    lines = ['#include <cstdio>', '#include <cstddef>', '#include "hvo.h"', 'int main() {']
    for ctype, mirror in hvo.RECORDS.items():
        lines.append('  std::printf("%s - %%zu 0\\n", sizeof(%s));' % (ctype, ctype))
        for k, _, _ in _fields(mirror):
            h = hvo.HEADER_NAMES.get(k, k)                    # (the header's name where the binding's differs)
            lines.append('  std::printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (ctype, k, ctype, h, ctype, h))
    lines += ['  return 0;', '}']
    d = tmp_path_factory.mktemp("layout")
    src = d / "layout.cpp"; src.write_text("\n".join(lines) + "\n")
    exe = d / "layout"
    tried = []
    for cc in COMPILERS:
        if shutil.which(cc[0]) is None:
            tried.append(cc[0] + ": not found"); continue
        r = subprocess.run(cc + ["-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
        if r.returncode == 0:
            break
        tried.append(" ".join(cc) + ": " + r.stderr[-2000:])
    else:
        pytest.fail("no host compiler built the layout program:\n" + "\n".join(tried))
    out = {}
    for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        ctype, field, a, b = ln.split()
        if field == "-":
            out[ctype] = (int(a), {})
        else:
            out[ctype][1][field] = (int(a), int(b))
    return out


def test_every_mirror_matches_the_header(hvo, header_layout):
    wrong = []
    for ctype, mirror in hvo.RECORDS.items():
        size, fields = header_layout[ctype]
        if _sizeof(mirror) != size:
            wrong.append("%s: sizeof %d, the header's %d" % (ctype, _sizeof(mirror), size))
        for k, off, sz in _fields(mirror):
            if (off, sz) != fields[k]:
                wrong.append("%s.%s: offset %d size %d, the header's %d %d" % (ctype, k, off, sz, *fields[k]))
    assert not wrong, "\n".join(wrong)


def test_every_mirror_is_in_the_table(hvo):
    """every ctypes.Structure subclass and every structured dtype of the package's modules appears in RECORDS"""
    listed = list(hvo.RECORDS.values())
    missing = []
    for f in sorted(os.listdir(PKG_DIR)):
        if not f.endswith(".py"):
            continue
        mod = hvo if f == "__init__.py" else importlib.import_module("hvo_amd." + f[:-3])
        for name, v in vars(mod).items():
            if inspect.isclass(v) and issubclass(v, ctypes.Structure) and v is not ctypes.Structure and v.__module__.startswith("hvo_amd"):
                if v not in listed: missing.append("%s.%s" % (mod.__name__, name))
            elif isinstance(v, np.dtype) and v.names and not any(v is m for m in listed):
                missing.append("%s.%s" % (mod.__name__, name))
    assert not missing, missing
    assert len(set(hvo.RECORDS)) == len(listed) and len({id(m) for m in listed}) == len(listed)
