"""Robustness of the host FLAC decoder (csrc/flac.cpp) on input it did not write: tests/native/flac_harness.cpp,
a stand-alone program compiled together with flac.cpp by the host compiler ($CXX, default g++) and run on a small
corpus from tests/flac_writer.py.  See the harness for its four properties (random mutation, every single-bit flip,
every prefix, hand-made headers and frames).

Two builds: plain -O2 (runs everywhere), and -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all, where any
report of either sanitizer ends the program with a non-zero status.  The instrumented program is a host program for a
CPU machine: it is skipped where the compiler or its sanitizer runtimes are missing and on any machine with a GPU
driver node (/dev/kfd).  Nothing is loaded into Python.  CPU only."""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

import flac_writer
from flac_writer import encode

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HARNESS = os.path.join(HERE, "native", "flac_harness.cpp")
FLAC = os.path.join(REPO, "audiotokenization_amd", "csrc", "flac.cpp")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
N = 6000  # mutated decodes per stream: the instrumented run of the whole corpus stays well under a minute

KINDS = [dict(kind="verbatim"), dict(kind="constant")] + [dict(kind="fixed", order=o) for o in range(5)] + \
        [dict(kind="lpc", order=o, lpc_prec=p) for o, p in ((1, 12), (2, 15), (8, 12), (32, 10))]


def _signal(C, T, bps, seed):
    rng = np.random.default_rng(seed)
    lim = (1 << (bps - 1)) - 1
    t = np.arange(T)
    x = np.sin(2 * np.pi * t * (0.013 + 0.004 * np.arange(C)[:, None])) * 0.6 * lim + rng.normal(0, lim * 0.01, (C, T))
    return np.clip(np.round(x), -lim - 1, lim).astype(np.int64)


def _corpus(d):
    """The flip stream first (stereo 16-bit, 3 frames, total known), then streams that between them hold every
    subframe kind, 8 / 16 / 24 / 32-bit samples, 1 / 2 / 8 channels, every channel assignment, Rice (4- and 5-bit
    parameters) and escaped partitions, wasted bits and variable block sizes; a few hundred samples each."""
    flac_writer.EMITTED.clear()
    assigns, paths = set(), []

    def write(name, x, bps, sizes, plan, **kw):
        p = os.path.join(d, name)
        with open(p, "wb") as fh:
            fh.write(encode(x, 16000, bps, block_sizes=sizes, plan=plan, **kw))
        paths.append(p)

    def flip_plan(fi, c):
        if fi == "stereo":
            return (10, 8, 9)[c % 3]
        return (dict(kind="lpc", order=4, porder=1), dict(kind="fixed", order=2, porder=2, method=1),
                dict(kind="verbatim"))[(fi + c) % 3]

    write("flip.flac", _signal(2, 150, 16, 1), 16, [64, 32, 54], flip_plan)
    i = 0
    for C, bps in ((1, 8), (2, 16), (1, 24), (2, 32), (8, 16), (2, 8), (2, 24), (1, 32), (1, 16)):
        T = 300 if C < 8 else 120
        x = _signal(C, T, bps, 10 + i)
        wasted = 2 if i % 3 == 1 else 0
        if wasted:
            x = x // 4 * 4
        sizes = [64, 16, 96, 48]
        starts = np.cumsum([0] + sizes * 4)
        for fi in range(len(starts) - 1):  # a constant block wherever the plan asks for a CONSTANT subframe
            if any(KINDS[(fi * C + c + i) % len(KINDS)]["kind"] == "constant" for c in range(C)):
                x[:, starts[fi]:starts[fi + 1]] = (3 - fi) * 4

        def plan(fi, c, i=i, C=C, bps=bps, wasted=wasted):
            if fi == "stereo":
                a = (1, 8, 9, 10)[(c + i) % 4]
                assigns.add(a)
                return a
            k = dict(KINDS[(fi * C + c + i) % len(KINDS)])
            esc = (0,) if (fi + i) % 3 == 0 and bps < 32 else ()  # an escaped residual holds 31 bits at the most
            k.update(porder=fi % 4, method=(fi + c) % 2, escape_parts=esc, wasted=wasted)
            return k

        write(f"c{i}.flac", x, bps, sizes, plan, variable=bool(i % 2), extra_meta=bool(i % 3))
        i += 1
    em = flac_writer.EMITTED
    kinds = {(k, o) for k, o, *_ in em}
    assert {("verbatim", 0), ("constant", 0)} | {("fixed", o) for o in range(5)} <= kinds, kinds
    assert {("lpc", o) for o in (1, 2, 8, 32)} <= kinds, kinds
    assert any(e[2] for e in em) and {e[3] for e in em if e[0] in ("fixed", "lpc")} == {0, 1} and any(e[4] for e in em)
    assert assigns == {1, 8, 9, 10}
    return paths


def _cxx():
    return os.environ.get("CXX", "g++")


def _compile(out, flags, sources):
    return subprocess.run([_cxx(), "-std=c++17", *flags, *sources, "-o", out], capture_output=True, text=True)


def _run(exe, corpus, env=None):
    t0 = time.perf_counter()
    res = subprocess.run([exe, str(N), *corpus], capture_output=True, text=True, env=env)
    print(res.stdout + res.stderr)
    print(f"{os.path.basename(exe)}: {N} mutated decodes of each of {len(corpus)} streams, "
          f"{time.perf_counter() - t0:.1f} s")
    return res


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return _corpus(str(tmp_path_factory.mktemp("flac_corpus")))


def test_harness_plain(corpus, tmp_path):
    assert shutil.which(_cxx()), f"{_cxx()}: the host compiler that builds the ops library is missing"
    exe = str(tmp_path / "flac_harness")
    res = _compile(exe, ["-O2"], [HARNESS, FLAC])
    assert res.returncode == 0, res.stderr
    res = _run(exe, corpus)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "none accepted" in res.stdout and f"{N * len(corpus)} decodes" in res.stdout


def test_harness_under_asan_and_ubsan(corpus, tmp_path):
    if os.path.exists("/dev/kfd"):
        pytest.skip("a machine with a GPU driver node: the instrumented host program runs on CPU machines only")
    if not shutil.which(_cxx()):
        pytest.skip(f"{_cxx()} not found")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    res = _compile(str(tmp_path / "probe"), SAN, [str(probe)])
    if res.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        print(res.stderr)
        pytest.skip(f"{_cxx()} cannot build or start a program with -fsanitize=address,undefined here")
    exe = str(tmp_path / "flac_harness_san")
    res = _compile(exe, SAN, [HARNESS, FLAC])
    assert res.returncode == 0, res.stderr
    # the harness frees what it allocates; leak checking needs ptrace, which containers may forbid
    res = _run(exe, corpus, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert res.returncode == 0, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
    assert "none accepted" in res.stdout and f"{N * len(corpus)} decodes" in res.stdout
