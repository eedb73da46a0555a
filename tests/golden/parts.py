"""Golden fixtures above the size a committed file may have are stored in numbered parts,
``<stem>.part<i>.npz``: each part a complete .npz that holds a run of the fixture's arrays.
``load`` reads a fixture in either form and hands back what ``np.load`` would (``files``,
``fixture[key]``, ``key in fixture``); ``save`` writes one, split only when it has to be."""
import glob
import io
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_BYTES = 1_000_000  # per file, below the 1 MiB a committed file may have


class Fixture:
    def __init__(self, arrays):
        self._arrays = arrays
        self.files = list(arrays)

    def __getitem__(self, key):
        return self._arrays[key]

    def __contains__(self, key):
        return key in self._arrays

    def __iter__(self):
        return iter(self.files)


def part_paths(name, here=HERE):
    stem = name[:-len(".npz")]
    paths = glob.glob(os.path.join(here, glob.escape(stem) + ".part*.npz"))
    num = re.compile(re.escape(stem) + r"\.part(\d+)\.npz$")
    paths = [p for p in paths if num.search(os.path.basename(p))]
    return sorted(paths, key=lambda p: int(num.search(os.path.basename(p)).group(1)))


def load(name, here=HERE):
    """`name` ("transformer.npz") as one mapping, from the file itself or from its parts."""
    paths = part_paths(name, here) or [os.path.join(here, name)]
    arrays = {}
    for p in paths:
        with np.load(p) as z:
            for k in z.files:
                arrays[k] = z[k]
    return Fixture(arrays)


def _compressed(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getvalue()


def save(name, arrays, here=HERE):
    """Write `arrays` as `name`, or as the fewest parts (runs of the arrays in their order) that each stay under
    MAX_BYTES.  Returns the paths written; a stale whole file or stale parts of the same fixture are removed."""
    keys = list(arrays)
    for n in range(1, len(keys) + 1):
        total = sum(np.asarray(arrays[k]).nbytes for k in keys) or 1
        groups, cur, acc = [], [], 0
        for k in keys:  # contiguous runs of about total / n bytes each
            if cur and acc >= total * len(groups + [cur]) / n:
                groups.append(cur)
                cur = []
            cur.append(k)
            acc += np.asarray(arrays[k]).nbytes
        groups.append(cur)
        blobs = [_compressed({k: arrays[k] for k in g}) for g in groups]
        if all(len(b) <= MAX_BYTES for b in blobs):
            break
    else:
        raise ValueError(f"{name}: one array alone is larger than {MAX_BYTES} bytes compressed")
    stale = part_paths(name, here) + [os.path.join(here, name)]
    for p in stale:
        if os.path.exists(p):
            os.remove(p)
    stem = name[:-len(".npz")]
    paths = [os.path.join(here, name)] if len(blobs) == 1 else \
            [os.path.join(here, f"{stem}.part{i}.npz") for i in range(len(blobs))]
    for p, b in zip(paths, blobs):
        with open(p, "wb") as f:
            f.write(b)
    return paths
