"""Generate tests/golden/perplexity_cases.npz from the REFERENCE's calculate_perplexity (inference_full.py:570-604).

Run in the development container only (the reference never travels):
    python tools/make_golden_perplexity.py
inference_full.py cannot be imported here (librosa, torchmetrics, ... are absent), so that one function's
definition is taken out of the file's syntax tree and executed on its own with numpy.
Fixture = data: three usage counters (uniform, one-hot, a seeded skewed one that also has keys at and beyond the
codebook size, which the function leaves out of the distribution but keeps in the total), each as the in-range
counts, the total over all keys, and the function's (normalized, raw) answer.
"""
from __future__ import annotations

import ast
import os
import sys
from collections import Counter

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import refimport  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "perplexity_cases.npz")


def load_calculate_perplexity():
    path = os.path.join(refimport.REF_ROOT, "inference_full.py")
    with open(path) as fh:
        tree = ast.parse(fh.read(), path)
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "calculate_perplexity")
    ns = {"np": np}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns["calculate_perplexity"]


def main():
    calc = load_calculate_perplexity()
    size = 64
    rng = np.random.default_rng(11)
    skew = Counter({int(k): int(v) for k, v in zip(rng.permutation(size)[:40], rng.geometric(0.02, 40))})
    skew.update({size: 7, size + 5: 3, 10 * size: 11})  # out of range: ignored, but counted in the total
    cases = {"uniform": Counter({k: 5 for k in range(size)}), "onehot": Counter({17: 123}), "skewed": skew}
    out = {"codebook_size": np.int64(size)}
    for name, counter in cases.items():
        norm, raw = calc(counter, size)
        counts = np.zeros(size, np.int64)
        for k, v in counter.items():
            if 0 <= k < size:
                counts[k] = v
        out[name + "_counts"] = counts
        out[name + "_total"] = np.int64(sum(counter.values()))
        out[name + "_expected"] = np.array([norm, raw], np.float64)
        print(name, int(out[name + "_total"]), norm, raw)
    np.savez(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
