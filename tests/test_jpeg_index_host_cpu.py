"""The entry-point decoder of csrc/ssdhip_jpeg_entropy.h compiled for the HOST (tests/jpeg_index_main.cpp, built here with the host
compiler and run as a program): recording a file's entries, decoding through them, and what tampered entries and corrupted bytes do --
against ssdhip_jpeg_decode_segment in the same program and against the NumPy restatement (tests/np_jpeg.py).  Plus the Python side
that needs no GPU: `JpegIndex` files and the entry table `pack_plans` writes.  No sanitizer flags here; the same program builds with
-fsanitize=address,undefined for a run by hand on the CPU (every part of a case is an exact-size heap block there)."""
import copy
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import np_jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD, INDEXED = 0, 1


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("jpeg_index") / "jpeg_index_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "ssd_keras_amd", "csrc"),
                           os.path.join(ROOT, "tests", "jpeg_index_main.cpp"), "-o", exe])
    return exe


def _case(plan, data, op, entries):
    """One case of the program's input: the descriptor buffer of a one-image batch, the operation, the entry table (absolute
    offsets in the batch's bytes, which for one image are the offsets from the start of the scan's bytes)."""
    from ssd_keras_amd.data_generator.jpeg_decode import pack_plans
    host, a, _ = pack_plans([plan], [data])
    assert a["n_images"] == 1 and a["n_segments"] == 1
    entries = np.ascontiguousarray(entries, dtype=np.int32).reshape(-1, 8)
    rows = plan.mcuy if op == RECORD else 0
    head = struct.pack("<16i", 0x4A504958, a["n_huff"], a["off_images"], a["off_segments"], a["off_huff"], a["off_data"], a["data_bytes"],
                       a["total_blocks"], len(host), op, len(entries), rows, 0, 0, 0, 0)
    return head + host.tobytes() + entries.tobytes(), a["total_blocks"], rows


def run_cases(program, cases, tmp_path):
    """cases [(plan, bytes, op, entries)] -> [(sequential status, status, sequential coef, coef, recorded entries)], one run of the
    program, inside a time limit."""
    blobs = [_case(*c) for c in cases]
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<i", len(blobs)))
        for blob, _, _ in blobs:
            f.write(blob)
    subprocess.run([program, src, dst], check=True, timeout=120)
    raw = open(dst, "rb").read()
    out, pos = [], 0
    for _, blocks, rows in blobs:
        seq_status, status = struct.unpack_from("<2i", raw, pos)
        seq = np.frombuffer(raw, dtype=np.int16, count=blocks * 64, offset=pos + 8).reshape(blocks, 64)
        coef = np.frombuffer(raw, dtype=np.int16, count=blocks * 64, offset=pos + 8 + blocks * 128).reshape(blocks, 64)
        ckpt = np.frombuffer(raw, dtype=np.int32, count=rows * 8, offset=pos + 8 + blocks * 256).reshape(rows, 8)
        out.append((seq_status, status, seq, coef, ckpt))
        pos += 8 + blocks * 256 + rows * 32
    assert pos == len(raw)
    return out


def _reference(plan, data):
    ref = np_jpeg.parse(data[:plan.segments[0][0]] + b"\xff\xd9")      # the headers; the ranges are the plan's
    ref.segments = list(plan.segments)
    return np_jpeg.entropy(data, ref)


def _record(program, files, tmp_path):
    """[(plan, recorded entries)] of clean files."""
    from ssd_keras_amd.data_generator.jpeg_decode import plan_jpeg
    plans = [plan_jpeg(d) for d in files]
    got = run_cases(program, [(p, d, RECORD, []) for p, d in zip(plans, files)], tmp_path)
    assert all(g[1] == 0 for g in got)
    return [(p, g[4].copy()) for p, g in zip(plans, got)]


def test_clean_files(program, tmp_path):
    """Recording gives the sequential coefficients and one entry per MCU row; decoding through those entries gives them again."""
    from ssd_keras_amd.data_generator.jpeg_decode import plan_jpeg
    members = [(k, d) for k, d in np_jpeg.grid() if k[5] == 0]
    assert len(members) == 224
    members += [((120, 160, s, q), np_jpeg.make_jpeg(120, 160, s, q)) for s in (0, 1, 2, "L") for q in (30, 95)]
    plans = [plan_jpeg(d) for _, d in members]
    assert all(p is not None and p.restart_interval == 0 and len(p.segments) == 1 for p in plans)
    recorded = run_cases(program, [(p, d, RECORD, []) for p, (_, d) in zip(plans, members)], tmp_path)
    single = 0
    for (key, data), plan, (seq_status, status, seq, coef, ckpt) in zip(members, plans, recorded):
        want, want_status = _reference(plan, data)
        assert status == seq_status == want_status == 0, key
        assert np.array_equal(coef, seq) and np.array_equal(coef, want), key
        assert ckpt.shape == (plan.mcuy, 8), key
        assert np.array_equal(ckpt[:, 3], np.arange(plan.mcuy) * plan.mcux) and (ckpt[:, 4] == plan.mcux).all(), key
        assert tuple(ckpt[0]) == (0, 0, 0, 0, plan.mcux, 0, 0, 0), key
        assert ((ckpt[:, 2] >= 0) & (ckpt[:, 2] <= 7)).all() and (np.diff(ckpt[:, 1]) >= 0).all(), key
        lo, hi = plan.segments[0]
        for byte in ckpt[:, 1]:                                  # never the 00 of an FF 00 pair
            assert 0 <= byte <= hi - lo and not (byte > 0 and byte < hi - lo and data[lo + byte] == 0 and data[lo + byte - 1] == 0xFF), key
        single += plan.mcuy == 1
    assert single >= 8                                           # single-MCU-row files: an index of one entry (checked by the shape above)
    indexed = run_cases(program, [(p, d, INDEXED, r[4]) for p, (_, d), r in zip(plans, members, recorded)], tmp_path)
    for (key, _), rec, (seq_status, status, seq, coef, _) in zip(members, recorded, indexed):
        assert status == seq_status == 0, key
        assert np.array_equal(coef, seq) and np.array_equal(coef, rec[3]), key


def _three_files():
    return [np_jpeg.make_jpeg(33, 50, 2, 95, False, 0, seed=11), np_jpeg.make_jpeg(40, 41, 0, 75, True, 0, seed=12),
            np_jpeg.make_jpeg(48, 64, "L", 100, False, 0, seed=13)]


def test_tampered_indices(program, tmp_path):
    """Every single change to a recorded index is noticed: a non-zero status, whatever else the lanes decoded."""
    files = _three_files()
    cases, names = [], []
    for data, (plan, rows) in zip(files, _record(program, files, tmp_path)):
        n = len(rows)
        assert n >= 3
        lo, hi = plan.segments[0]

        def add(name, row, col, delta=None, value=None):
            bad = rows.copy()
            bad[row, col] = bad[row, col] + delta if value is None else value
            cases.append((plan, data, INDEXED, bad))
            names.append((name, row))

        for row in range(1, n):
            for delta in (-1, 1):
                add("bit %+d" % delta, row, 2, delta)
                add("byte %+d" % delta, row, 1, delta)
                add("pred0 %+d" % delta, row, 5, delta)
        add("pred0 of the first entry", 0, 5, 1)
        add("bit of the first entry", 0, 2, 1)
        add("byte of the first entry", 0, 1, 1)
        if plan.ncomp == 3:
            add("pred1", 1, 6, 1)
            add("pred2", n - 1, 7, -1)
        for a, b in ((0, 1), (1, 2), (n - 2, n - 1)):
            bad = rows.copy()
            bad[[a, b]] = bad[[b, a]]
            cases.append((plan, data, INDEXED, bad))
            names.append(("swapped", a))
        cases.append((plan, data, INDEXED, rows[:-1]))           # an index that stops short of the image
        names.append(("short", n - 1))
        cases.append((plan, data, INDEXED, rows[1:]))            # and one that starts late
        names.append(("late", 0))
        # out of range: no access outside the parts (a sanitizer build of the program proves it; here: a status, and the run ends)
        for value in (hi - lo + 1, 2 ** 31 - 1, -1, -2 ** 31):
            add("byte %d" % value, 1, 1, value=value)
        for value in (-1, plan.mcux * plan.mcuy, 2 ** 31 - 1, -2 ** 31):
            add("first_mcu %d" % value, 1, 3, value=value)
        for value in (0, -1, plan.mcux * plan.mcuy, 2 ** 31 - 1, -2 ** 31):
            add("n_mcus %d" % value, 1, 4, value=value)
        for value in (8, -1, 2 ** 31 - 1):
            add("bit %d" % value, 1, 2, value=value)
    for name, (seq_status, status, _, _, _) in zip(names, run_cases(program, cases, tmp_path)):
        assert seq_status == 0 and status != 0, name


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


def test_corrupted_data_with_the_clean_index(program, tmp_path):
    """200 seeded corruptions of three files, decoded through the index of the CLEAN file: status 0 only where the sequential decode
    of the corrupted bytes has status 0 too, and then with its coefficients."""
    files = _three_files()
    rng = np.random.RandomState(2024)
    cases = []
    for data, (plan, rows), n in zip(files, _record(program, files, tmp_path), (67, 67, 66)):
        cases += [(p, d, INDEXED, rows) for p, d in corruptions(data, plan, rng, n)]
    assert len(cases) == 200
    seen = set()
    for k, (seq_status, status, seq, coef, _) in enumerate(run_cases(program, cases, tmp_path)):
        if status == 0:
            assert seq_status == 0, k
            assert np.array_equal(coef, seq), k
            want, want_status = _reference(cases[k][0], cases[k][1])
            assert want_status == 0 and np.array_equal(coef, want), k
        seen.add(status != 0)
    assert seen == {False, True}                                 # some corruptions decode to the end through the index, some are caught


# ---- the Python side ------------------------------------------------------------------------------------------------------------------
def test_jpeg_index_file_round_trip(tmp_path):
    from ssd_keras_amd.data_generator.jpeg_decode import JpegIndex
    rng = np.random.RandomState(5)
    ix = JpegIndex()
    name_key = JpegIndex.key("/data/VOC/JPEGImages/000001.jpg", b"x" * 1234)
    bytes_key = JpegIndex.key(b"abc", b"abc")
    assert name_key != JpegIndex.key("/data/VOC/JPEGImages/000001.jpg", b"x" * 1235) and bytes_key != JpegIndex.key(b"abd", b"abd")
    for key, rows in ((name_key, 24), (bytes_key, 2), ("f:7:with spaces, and ünicode.jpg", 47)):
        ix[key] = rng.randint(-2 ** 31, 2 ** 31, size=(rows, 8), dtype=np.int64).astype(np.int32)
    path = str(tmp_path / "index.npz")
    ix.save(path)
    with np.load(path, allow_pickle=False) as z:                 # plain arrays only
        assert sorted(z.files) == ["counts", "keys", "rows"] and z["rows"].dtype == np.int32 and z["rows"].shape == (73, 8)
    back = JpegIndex.load(path)
    assert back.keys() == ix.keys() and len(back) == 3
    for key in ix.keys():
        assert back[key].dtype == np.int32 and np.array_equal(back[key], ix[key])
    empty = str(tmp_path / "empty.npz")
    JpegIndex().save(empty)
    assert len(JpegIndex.load(empty)) == 0
    small = JpegIndex(max_files=2)                               # the bound drops the oldest
    for key in ix.keys():
        small[key] = ix[key]
    assert small.keys() == ix.keys()[1:]
    small.clear()
    assert len(small) == 0 and name_key not in small


def test_entry_table_packing(program, tmp_path):
    """`pack_plans(index_rows=...)`: without the keyword nothing changes; with it the buffer gains mode words and the entry table in
    struct ssdhip_jpeg_entry's layout -- which the host program, reading the packed bytes as that struct, confirms by decoding."""
    from ssd_keras_amd.data_generator.jpeg_decode import RECORD as REC, pack_plans, plan_jpeg
    files = _three_files() + [np_jpeg.make_jpeg(24, 40, 2, 85, restart=4, seed=25)]
    recorded = _record(program, files[:3], tmp_path)
    plans = [p for p, _ in recorded] + [plan_jpeg(files[3])]
    rows = [recorded[0][1], REC, recorded[2][1], None]
    plain, plain_args, plain_outs = pack_plans(plans, files)
    host, a, outs = pack_plans(plans, files, index_rows=rows)
    assert outs == plain_outs and all(a[k] == v for k, v in plain_args.items())
    assert np.array_equal(host[:len(plain)], plain) and len(host) > len(plain)
    assert a["off_modes"] % 16 == 0 and a["off_entries"] % 16 == 0 and a["off_modes"] >= a["off_status"] + 4 * len(plans)
    segments = host[a["off_segments"]:a["off_segments"] + 16 * a["n_segments"]].view(np.int32).reshape(-1, 4)
    modes = host[a["off_modes"]:a["off_modes"] + 4 * len(plans)].view(np.int32)
    assert list(modes & 3) == [1, 2, 1, 0]
    assert modes[1] >> 2 == 0 and a["ckpt_entries"] == plans[1].mcuy and a["ckpt_base"] == [None, 0, None, None]
    assert a["record_segments"] == 1 + len(plans[3].segments)
    table = host[a["off_entries"]:a["off_entries"] + 32 * a["n_entries"]].view(np.int32).reshape(-1, 8)
    assert a["n_entries"] == len(rows[0]) + len(rows[2]) and a["off_entries"] + 32 * a["n_entries"] <= len(host)
    at = 0
    for i in (0, 2):
        mine = table[at:at + len(rows[i])]
        at += len(rows[i])
        seg = segments[modes[i] >> 2]
        assert seg[0] == i and (mine[:, 0] == i).all()
        assert np.array_equal(mine[:, 1], rows[i][:, 1] + seg[1]) and np.array_equal(mine[:, 2:], rows[i][:, 2:])
    # one image, so that the packed table is what the program's lanes read: image, byte, bit, first_mcu, n_mcus, pred0, pred1, pred2
    host1, a1, _ = pack_plans(plans[:1], files[:1], index_rows=rows[:1])
    table1 = host1[a1["off_entries"]:a1["off_entries"] + 32 * a1["n_entries"]].view(np.int32).reshape(-1, 8)
    (seq_status, status, seq, coef, _), = run_cases(program, [(plans[0], files[0], INDEXED, table1)], tmp_path)
    assert status == seq_status == 0 and np.array_equal(coef, seq)
