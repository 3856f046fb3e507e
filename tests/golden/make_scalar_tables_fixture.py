"""Generator of tests/golden/scalar_tables.npz: a digest of every flat table the flattener makes of every scene in
tests/scenes.py ALL_SCENES (BLAKE2b-128 over dtype, shape and bytes, per field of CompiledScene.TABLE_FIELDS, plus
root_id and total_bins).  Made on the commit before refractive-index tables, it pins that a scene whose indices are
numbers still compiles to exactly the arrays it compiled to then (tests/test_dispersion.py).  keys: 'scene/field'; digests: one row of 16 bytes per key.

    python tests/golden/make_scalar_tables_fixture.py OUT.npz
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def digest(array):
    a = np.ascontiguousarray(array)
    h = hashlib.blake2b(digest_size=16)
    h.update(a.dtype.str.encode()); h.update(repr(a.shape).encode()); h.update(a.data if a.size else b"")
    return np.frombuffer(h.digest(), dtype=np.uint8)


def table_digests(compiled, fields):
    out = {name: digest(getattr(compiled, name)) for name in fields}
    out["root_id"] = digest(np.int64(compiled.root_id))
    out["total_bins"] = digest(np.int64(compiled.total_bins))
    return out


def main(path):
    from pvtrace_amd.engine import compile_scene
    from tests import scenes

    keys, digests = [], []
    for name in sorted(scenes.ALL_SCENES):
        c = compile_scene(scenes.ALL_SCENES[name]())
        for field, value in table_digests(c, c.TABLE_FIELDS).items():
            keys.append(f"{name}/{field}")
            digests.append(value)
    np.savez_compressed(path, keys=np.array(keys), digests=np.array(digests))
    print(f"{path}: {len(keys)} digests")


if __name__ == "__main__":
    main(sys.argv[1])
