"""The marshalling core of the binding: how a call's arrays reach a ctypes record and come back.  A binding record is declared once, as

  an Inputs table   rows (field, dtype, trailing shape, REQ | OPT, length group) -> fill() makes the arrays contiguous, points the record
                    at them (NULL for None and for empty), checks the lengths of a group and returns what must stay alive;
  an Outputs table  rows (field, dtype, columns, which length it has, which count cuts it) with the family's sentinel -> alloc() makes
                    max(n, 1) rows of sentinel per array and points the record at them, finish() cuts them after the call;
  a return path     returned(), the check=True / check=False protocol of every call that can be refused.

Pure numpy and ctypes: nothing here loads the library, so tests/test_binding_marshal.py runs without a device."""
import ctypes as C
import numpy as np

REQ, OPT = True, False


def ptr(a):
    """the address of an array, NULL for None and for an empty one (an empty array has no address worth passing)"""
    return a.ctypes.data if a is not None and a.size else None


def as_bytes(v):
    """a flag array as 0 / 1 bytes, whatever it was given as"""
    return np.ascontiguousarray(np.asarray(v).astype(bool), np.uint8)


def vec(dst, src, n=None):
    """a small float vector field (Tcw[12], bounds[4], cam[6]) from any sequence: all of dst, or its first n from the first n of src"""
    v = np.asarray(src, np.float32).reshape(len(dst) if n is None else -1)
    for k in range(len(dst) if n is None else n):
        dst[k] = v[k]


def bounds(dst, bounds4):
    """bounds[4] = (min x, max x, min y, max y); None: the resident frame's own grid is used and the field holds (0, 1, 0, 1)"""
    vec(dst, (0.0, 1.0, 0.0, 1.0) if bounds4 is None else bounds4)


class Inputs:
    """rows: (field, dtype (bool: flags, sent as bytes), trailing shape, REQ | OPT, length group).  The group "n" is the record's own count,
    taken from the first "n" row (or from `count_from`, or given); None is a free length; any other name is a length the caller passes to
    fill().  With `differ`, REQ rows of "n" may have any length and a disagreement raises ValueError(differ); every other grouped row is
    reshaped to its length, which raises numpy's own error."""

    def __init__(self, rows, count="n", differ=None, count_from=None):
        self.rows, self.count, self.differ = tuple(rows), count, differ
        self.count_from = count_from or next((r[0] for r in rows if r[4] == "n"), None)

    def fill(self, rec, src, n=None, only=None, **lens):
        """src: a dict (an OPT key may be missing or None) -> (the arrays by field, n).  only: fill just these fields and leave the count"""
        a = {}
        for f, dt, trail, need, grp in self.rows:
            if only is not None and f not in only:
                continue
            v = src[f] if need else src.get(f)
            if v is None and not need:
                a[f] = None; continue
            v = as_bytes(v) if dt is bool else np.ascontiguousarray(v, dt)
            want = n if grp == "n" else lens.get(grp)
            checked = grp == "n" and need and self.differ
            v = v.reshape(((-1 if want is None or checked else want),) + tuple(trail))
            if f == self.count_from and n is None:
                n = len(v)
            elif checked and len(v) != n:
                raise ValueError(self.differ)
            a[f] = v
        n = 0 if n is None else n
        for f, v in a.items():
            setattr(rec, f, ptr(v))
        if self.count and only is None:
            setattr(rec, self.count, n)
        return a, n


class Outputs:
    """rows: (field, dtype, columns, length, cut).  length names the count the array is sized by (alloc(rec, n=..., n_frame=...));
    cut is None for a per-entry array (cut to its length) or the record's count field for a compacted list (cut to clamp(count, 0,
    length); (field, k) adds k).  sentinel fills every array (fill: per-field exceptions) and every field of `counts`; `scalars` are the
    record's fields finish() returns beside the arrays; copy: return copies, not views."""

    def __init__(self, rows, sentinel, counts=(), scalars=(), fill=None, copy=False):
        self.rows, self.sentinel, self.counts, self.scalars, self.fill, self.copy = tuple(rows), sentinel, tuple(counts), tuple(scalars), fill or {}, copy

    def alloc(self, rec, want=None, **lens):
        """-> the arrays by field.  want: only these fields are given to the record, the others go as NULL (their arrays are still made)"""
        a = {}
        for f, dt, cols, length, _ in self.rows:
            m = max(int(lens[length]), 1)
            a[f] = np.full((m, cols) if cols > 1 else m, self.fill.get(f, self.sentinel), dt)
            setattr(rec, f, a[f].ctypes.data if want is None or f in want else None)
        for f in self.counts:
            setattr(rec, f, self.sentinel)
        return a

    def cut(self, rec, a, ok=True, **lens):
        """the arrays cut to the lengths / the record's counts; ok False (a refusal): whole, as the call left them"""
        d = {}
        for f, _, _, length, cut in self.rows:
            v = a[f]
            if ok:
                n = int(lens[length])
                if cut is not None:
                    field, more = cut if isinstance(cut, tuple) else (cut, 0)
                    n = max(0, min(getattr(rec, field) + more, n))
                v = v[:n]
            d[f] = v.copy() if self.copy else v
        return d

    def finish(self, rec, a, ok=True, **lens):
        d = {k: getattr(rec, k) for k in self.scalars}
        d.update({k: tuple(v) for k, v in d.items() if isinstance(v, C.Array)})
        d.update(self.cut(rec, a, ok, **lens))
        return d


def returned(rc, last_error, name, chk, finish, check=True, ok=0):
    """the end of every call that can be refused.  check: chk(rc, name) raises on a refusal, then finish(True) is returned; else
    (rc, the handle's message, finish(rc == ok)) whatever rc is.  A finish that returns a tuple is spliced into that tuple."""
    if check:
        chk(rc, name)
        return finish(True)
    r = finish(rc == ok)
    return (rc, last_error().decode()) + (r if isinstance(r, tuple) else (r,))
