"""The golden fixtures' file format (tests/golden/*.npz).  TEST INFRASTRUCTURE.

Every committed file stays under 1 MiB: save() writes an .npz whose members are LZMA-compressed (np.load reads it as
any .npz), and a set that is still larger is split by case over several files -- PARTS names them -- which load() merges
back into one mapping."""
import os
import zipfile

import numpy as np

PARTS = {"flow_layer": ("flow_layer", "flow_layer_pairs")}     # flow_layer_pairs: the cases with two warped coordinates


def save(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_LZMA) as z:
        for k, v in arrays.items():
            with z.open(k + ".npy", "w") as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)


def load(golden_dir, name):
    gold = {}
    for part in PARTS.get(name, (name,)):
        with np.load(os.path.join(golden_dir, part + ".npz")) as z:
            gold.update({k: z[k] for k in z.files})
    return gold
