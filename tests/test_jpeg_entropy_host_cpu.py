"""csrc/ssdhip_jpeg_entropy.h compiled for the HOST: the segment decoder the entropy kernel calls, built with the host compiler
around tests/jpeg_entropy_main.cpp and run as a program, against the NumPy restatement (tests/np_jpeg.py) -- coefficients and status
words, on clean files and on corrupted ones.  No sanitizer flags here; the same program builds with -fsanitize=address,undefined for
a run by hand on the CPU."""
import copy
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import np_jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("jpeg_entropy") / "jpeg_entropy_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "ssd_keras_amd", "csrc"),
                           os.path.join(ROOT, "tests", "jpeg_entropy_main.cpp"), "-o", exe])
    return exe


def _case(plan, data):
    """One case of the program's input: the descriptor buffer of a one-image batch."""
    from ssd_keras_amd.data_generator.jpeg_decode import pack_plans
    host, a, _ = pack_plans([plan], [data])
    head = struct.pack("<12i", 0x4A504547, a["n_images"], a["n_segments"], a["n_huff"], a["off_images"], a["off_segments"], a["off_huff"],
                       a["off_data"], a["data_bytes"], a["total_blocks"], len(host), 0)
    return head + host.tobytes(), a["total_blocks"]


def run_cases(program, cases, tmp_path):
    """cases [(plan, bytes)] -> [(status, coef int16 [blocks][64])], one run of the program, inside a time limit."""
    blobs = [_case(p, d) for p, d in cases]
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<i", len(blobs)))
        for blob, _ in blobs:
            f.write(blob)
    subprocess.run([program, src, dst], check=True, timeout=60)
    raw = open(dst, "rb").read()
    out, pos = [], 0
    for _, blocks in blobs:
        status = struct.unpack_from("<i", raw, pos)[0]
        coef = np.frombuffer(raw, dtype=np.int16, count=blocks * 64, offset=pos + 4).reshape(blocks, 64)
        out.append((status, coef))
        pos += 4 + blocks * 128
    assert pos == len(raw)
    return out


def _reference(plan, data):
    ref = np_jpeg.parse(data[:plan.segments[0][0]] + b"\xff\xd9")      # the headers; the ranges are the plan's
    ref.segments = list(plan.segments)
    return np_jpeg.entropy(data, ref)


def test_clean_files(program, tmp_path):
    from ssd_keras_amd.data_generator.jpeg_decode import plan_jpeg
    members = [(k, d) for k, d in np_jpeg.grid() if k[2] in (2, "L")]
    assert len(members) == 224
    cases = [(plan_jpeg(d), d) for _, d in members]
    for (key, data), (plan, _), (status, coef) in zip(members, cases, run_cases(program, cases, tmp_path)):
        want, want_status = _reference(plan, data)
        assert status == want_status == 0, key
        assert np.array_equal(coef, want), key


def corruptions(data, plan, rng, n):
    """n corrupted copies of a file as (plan, bytes): byte flips inside the entropy-coded bytes, truncations (the plan's ranges cut
    to what is left), an inserted FF D9.  The ranges stay those of the clean file: what the decoder does INSIDE them is the test."""
    lo, hi = plan.segments[0][0], plan.segments[-1][1]
    out = []
    for k in range(n):
        kind = k % 3
        bad, p = bytearray(data), copy.copy(plan)
        if kind == 0:
            for _ in range(int(rng.randint(1, 4))):
                bad[int(rng.randint(lo, hi))] = int(rng.randint(0, 256))
        elif kind == 1:
            cut = int(rng.randint(lo, hi))
            bad = bad[:cut]
            p.segments = [(min(b, cut), min(e, cut)) for b, e in plan.segments]
        else:
            at = int(rng.randint(lo, hi - 1))
            bad[at:at + 2] = b"\xff\xd9"
        out.append((p, bytes(bad)))
    return out


def test_corrupted_files(program, tmp_path):
    """200 seeded corruptions of three files: the same coefficients and the same status as the restatement, every run ends."""
    from ssd_keras_amd.data_generator.jpeg_decode import plan_jpeg
    files = [np_jpeg.make_jpeg(33, 50, 2, 95, False, 0, seed=11), np_jpeg.make_jpeg(40, 41, 2, 75, True, 2, seed=12),
             np_jpeg.make_jpeg(48, 64, "L", 100, False, 2, seed=13)]
    rng = np.random.RandomState(2024)
    cases = []
    for data, n in zip(files, (67, 67, 66)):
        cases += corruptions(data, plan_jpeg(data), rng, n)
    assert len(cases) == 200
    seen = set()
    for (plan, data), (status, coef) in zip(cases, run_cases(program, cases, tmp_path)):
        want, want_status = _reference(plan, data)
        assert status == want_status
        assert np.array_equal(coef, want)
        seen.add(status != 0)
    assert seen == {False, True}                                 # some corruptions decode to the end, some are caught
