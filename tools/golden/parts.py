"""Golden archives in parts: no committed file may exceed 1 MiB, so an archive whose compressed
.npz would is written as <name>.part<k>.npz files of at most PART_BYTES each.  An array too large
for one part is cut along axis 0 into pieces stored under "<key>@@<i>"; tests/test_golden.py::load
joins the parts (pieces concatenated in order), which gives back the arrays bit for bit.

Usage: python tools/golden/parts.py tests/golden/<name>.npz   (re-writes an existing archive in parts)
"""
import glob
import io
import os
import sys

import numpy as np

PART_BYTES = 900 * 1024     # per part file (the limit for a committed file is 1 MiB)
SEP = "@@"


def _packed(a):
    """Bytes `a` takes inside a compressed .npz (measured: compressibility varies by array)."""
    buf = io.BytesIO()
    np.savez_compressed(buf, a=a)
    return buf.getbuffer().nbytes


def _pieces(key, a):
    """[(stored key, array, packed bytes)]: `a` whole if it fits half a part, else cut along axis 0."""
    size = _packed(a)
    if size <= PART_BYTES // 2 or a.ndim == 0 or a.shape[0] < 2:
        return [(key, a, size)]
    n = min(a.shape[0], -(-size // (PART_BYTES // 3)))
    cuts = np.array_split(a, n, axis=0)
    return [(f"{key}{SEP}{i}", c, _packed(c)) for i, c in enumerate(cuts)]


def save(path, rec):
    """Write `rec` as path (one .npz) if that stays within PART_BYTES, else as parts next to it.
    Returns the files written."""
    stem = path[:-len(".npz")]
    for old in glob.glob(stem + ".part*.npz") + [path]:
        if os.path.exists(old):
            os.remove(old)
    np.savez_compressed(path, **rec)
    if os.path.getsize(path) <= PART_BYTES:
        return [path]
    os.remove(path)
    parts, room = [{}], PART_BYTES
    for key in rec:                                   # (keys stay in the archive's order)
        for k, a, size in _pieces(key, np.asarray(rec[key])):
            if size > room and parts[-1]:
                parts.append({})
                room = PART_BYTES
            parts[-1][k] = a
            room -= size
    files = []
    for i, p in enumerate(parts):
        files.append(f"{stem}.part{i}.npz")
        np.savez_compressed(files[-1], **p)
        assert os.path.getsize(files[-1]) < (1 << 20), (files[-1], os.path.getsize(files[-1]))
    return files


if __name__ == "__main__":
    for src in sys.argv[1:]:
        rec = dict(np.load(src, allow_pickle=False))
        for f in save(src, rec):
            print(f, os.path.getsize(f) // 1024, "KB")
