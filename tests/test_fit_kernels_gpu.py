"""csrc/ssdhip_fit.hip on the device against tests/np_fit.py: the meter's update bit for bit, the sum-of-squares partials bit for bit
where the arithmetic is exact and within the bound of the kernel's own order where it is not, the edges of its loads, and the
refusals."""
import ctypes

import numpy as np
import pytest

from tests import np_fit

pytestmark = pytest.mark.gpu

CHUNK = np_fit.CHUNK


def _nat():
    from ssd_keras_amd import _native as nat
    nat.load()
    return nat


def _block(fill=0):
    """A meter state block in the middle of a larger buffer: (whole buffer, the block's view, its offset)."""
    import torch
    nat = _nat()
    n = nat.fit_meter_state_bytes()
    assert n == nat.FIT_METER_STATE.itemsize == 48
    whole = torch.full((64 + n + 64,), fill, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 16 == 0
    return whole, whole[64:64 + n], 64


def _read(block):
    return _nat().fit_meter_parse(block.cpu().numpy())


def _same_bits(a, b):
    return np.asarray(a, dtype=np.float32).tobytes() == np.asarray(b, dtype=np.float32).tobytes()


def _check(block, ref):
    got = _read(block)
    assert np.float64(got["sum"]).tobytes() == np.float64(ref.sum).tobytes() or (np.isnan(got["sum"]) and np.isnan(ref.sum)), (got, ref.sum)
    assert (got["seen"], got["steps"], got["first_bad"]) == (ref.seen, ref.steps, ref.first_bad)
    assert _same_bits(got["last"], ref.last) or (np.isnan(got["last"]) and np.isnan(ref.last))


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("batch", [1, 3, 32])
def test_meter_hand_cases(batch):
    nat = _nat()
    rng = np.random.RandomState(batch)
    _, block, _ = _block()
    nat.fit_meter_reset(block)
    ref = np_fit.Meter()
    for step in range(4):
        loss = (rng.rand(batch) * 20 + 0.01).astype(np.float32)
        partials = (rng.rand(step * 700) * 300).astype(np.float32) if step else None      # none, then more than one staging tile
        l2 = 0.0 if partials is None else 5e-4
        nat.fit_meter_update(block, _cuda(loss), _cuda(partials) if partials is not None else None, l2)
        ref.update(loss, partials if partials is not None else (), l2)
        _check(block, ref)
    assert ref.seen == 4 * batch and ref.first_bad == -1


def test_meter_accumulates_in_float64():
    """A batch whose float32-accumulated sum loses every small term: 2^27, thirty ones, -2^27."""
    nat = _nat()
    loss = np.array([2.0 ** 27] + [1.0] * 30 + [-(2.0 ** 27)], dtype=np.float32)
    acc = np.float32(0)
    for v in loss:
        acc = np.float32(acc + v)
    ref = np_fit.Meter()
    assert ref.update(loss) == np.float32(30.0 / 32.0) != np.float32(acc / np.float32(32))
    # ... and partials whose float32 sum would stall: 2^24 followed by ones
    partials = np.array([2.0 ** 24] + [1.0] * 1500, dtype=np.float32)
    ref.update(loss, partials, 1.0)
    assert ref.last == np.float32(30.0 / 32.0) + np.float32(2.0 ** 24 + 1500)
    _, block, _ = _block()
    nat.fit_meter_reset(block)
    nat.fit_meter_update(block, _cuda(loss), None, 0.0)
    nat.fit_meter_update(block, _cuda(loss), _cuda(partials), 1.0)
    _check(block, ref)


def test_meter_latches_the_first_non_finite_step():
    nat = _nat()
    _, block, _ = _block()
    nat.fit_meter_reset(block)
    ref = np_fit.Meter()
    for step in range(6):
        loss = np.array([1.0, 2.0, 3.0], dtype=np.float32)
        if step == 2:
            loss[1] = np.nan
        if step == 4:
            loss[0] = np.inf
        nat.fit_meter_update(block, _cuda(loss), None, 0.0)
        ref.update(loss)
    got = _read(block)
    assert got["first_bad"] == 2 == ref.first_bad and not np.isfinite(got["sum"]) and got["steps"] == 6 and got["seen"] == 18
    assert _same_bits(got["last"], np.float32(2.0))
    # a non-finite PENALTY latches too (weights that became NaN), through the partials
    nat.fit_meter_reset(block)
    nat.fit_meter_update(block, _cuda(np.ones(3, np.float32)), _cuda(np.array([1.0, np.inf], np.float32)), 5e-4)
    assert _read(block)["first_bad"] == 0


def test_meter_reset_writes_the_whole_block_and_nothing_else():
    nat = _nat()
    whole, block, at = _block(fill=0xFF)
    nat.fit_meter_reset(block)
    raw = whole.cpu().numpy()
    want = np.zeros((), dtype=nat.FIT_METER_STATE)
    want["first_bad"] = -1
    assert raw[at:at + 48].tobytes() == want.tobytes()
    assert (raw[:at] == 0xFF).all() and (raw[at + 48:] == 0xFF).all()
    nat.fit_meter_update(block, _cuda(np.array([1.5, 2.5], np.float32)), _cuda(np.array([4.0], np.float32)), 0.5)
    raw = whole.cpu().numpy()
    assert (raw[:at] == 0xFF).all() and (raw[at + 48:] == 0xFF).all()
    got = _read(block)
    assert (got["sum"], got["seen"], got["steps"], got["first_bad"], float(got["last"])) == (8.0, 2, 1, -1, 4.0)


def test_meter_five_replays_equal_five_eager_updates():
    import torch
    nat = _nat()
    loss, partials = _cuda(np.array([0.1, 0.7, 1e-3], np.float32)), _cuda(np.array([3.0, 1e-7, 5.5], np.float32))
    _, eager, _ = _block()
    _, replayed, _ = _block()
    nat.fit_meter_reset(eager)
    nat.fit_meter_reset(replayed)
    for _ in range(5):
        nat.fit_meter_update(eager, loss, partials, 5e-4)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        nat.fit_meter_update(replayed, loss, partials, 5e-4)
    torch.cuda.synchronize()
    assert _read(replayed)["steps"] == 0                              # a capture runs nothing
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    assert eager.cpu().numpy().tobytes() == replayed.cpu().numpy().tobytes() and _read(replayed)["steps"] == 5


# ---- sum of squares ----------------------------------------------------------------------------------------------------------------
def _dtype(name):
    import torch
    return {"float32": torch.float32, "bfloat16": torch.bfloat16}[name]


def _run(tensors):
    import torch
    nat = _nat()
    table = nat.sumsq_table(tensors, tensors[0].device)
    out = torch.full((table[5],), float("nan"), dtype=torch.float32, device="cuda")
    nat.sumsq_partials(table, out)
    return out.cpu().numpy()


def _host(tensors):
    return [t.float().cpu().numpy().astype(np.float32) for t in tensors]


def _vector(name):
    return 8 if name == "bfloat16" else 4


SIZES = [1, 7, 63, 64, 65, CHUNK, CHUNK - 1, CHUNK + 1]


@pytest.mark.parametrize("name", ["float32", "bfloat16"])
def test_sumsq_small_integers_are_exact(name):
    """|w| <= 8 and a total below 2^24: every square, every partial and their total are integers float32 holds exactly, whatever the
    order of additions -- the partials must equal integer arithmetic bit for bit."""
    import torch
    rng = np.random.RandomState(3)
    tensors = [_cuda(rng.randint(-8, 9, size=n).astype(np.float32)).to(_dtype(name)) for n in SIZES]
    got = _run(tensors)
    want = np.array([np.sum(c.astype(np.int64) ** 2) for c in np_fit.chunks(_host(tensors))], dtype=np.int64)
    assert want.sum() < 2 ** 24 and len(want) == sum(-(-n // CHUNK) for n in SIZES) == 9
    assert got.tobytes() == want.astype(np.float32).tobytes()
    assert got.tobytes() == np_fit.sumsq_kernel_order(_host(tensors), _vector(name)).tobytes()
    assert float(got.astype(np.float64).sum()) == float(want.sum())


@pytest.mark.parametrize("name,offsets", [("float32", (4, 8, 12)), ("bfloat16", (2, 4, 6, 8, 14))])
def test_sumsq_tensors_off_the_16_byte_boundary(name, offsets):
    """Slices of a larger buffer that start 2, 4, 8, ... bytes past a 16-byte boundary, longer than a chunk and with a tail: the same
    partials, bit for bit, as the same values in an aligned tensor (the order of additions does not depend on the alignment), and as
    the kernel's order stated in NumPy; within the bound against float64."""
    import torch
    dt = _dtype(name)
    esz = 2 if name == "bfloat16" else 4
    rng = np.random.RandomState(5)
    n = CHUNK + 77
    data = _cuda(rng.randn(n).astype(np.float32) * 3).to(dt)
    aligned = _run([data, data[:19]])
    model = np_fit.sumsq_kernel_order(_host([data, data[:19]]), _vector(name))
    assert aligned.tobytes() == model.tobytes()
    truth = np_fit.sumsq_f64(_host([data, data[:19]]))
    assert (np.abs(aligned.astype(np.float64) - truth) <= np_fit.gamma(np_fit.DEPTH) * truth).all()
    for off in offsets:
        buf = torch.zeros((n + 64,), dtype=dt, device="cuda")
        view = buf[off // esz:off // esz + n]
        view.copy_(data)
        short = buf[off // esz:off // esz + 19]
        assert view.data_ptr() % 16 == off
        assert _run([view, short]).tobytes() == aligned.tobytes(), off


def test_sumsq_a_table_longer_than_one_launch():
    """129 tensors: one more than a launch's kernel arguments hold.  Integer data, exact."""
    rng = np.random.RandomState(7)
    tensors = [_cuda(rng.randint(-8, 9, size=5 + k % 7).astype(np.float32)) for k in range(129)]
    got = _run(tensors)
    want = np.array([np.sum(t.astype(np.int64) ** 2) for t in _host(tensors)], dtype=np.float32)
    assert got.shape == (129,) and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", ["float32", "bfloat16"])
def test_sumsq_random_data_within_the_bound_of_the_kernels_order(name):
    """All terms are non-negative, so a partial's relative error is at most gamma_d with d the longest chain of float32 roundings an
    element passes: d = 41 = the square, 31 additions in its lane, 6 across the lanes of its wave, 3 across the waves (np_fit.DEPTH).
    (A bf16 element is exact in float32: the bound is the same.)  Two runs are bit-identical, and equal the order stated in NumPy."""
    assert np_fit.DEPTH == 41
    rng = np.random.RandomState(11)
    tensors = [_cuda((rng.randn(n) * rng.choice([1e-3, 1.0, 50.0])).astype(np.float32)).to(_dtype(name)) for n in (3 * CHUNK + 5, 1000, CHUNK)]
    got, again = _run(tensors), _run(tensors)
    truth = np_fit.sumsq_f64(_host(tensors))
    assert got.shape == truth.shape == (6,)
    assert (np.abs(got.astype(np.float64) - truth) <= np_fit.gamma(np_fit.DEPTH) * truth).all()
    assert got.tobytes() == again.tobytes()
    assert got.tobytes() == np_fit.sumsq_kernel_order(_host(tensors), _vector(name)).tobytes()


def test_sumsq_a_nan_poisons_exactly_its_chunk():
    rng = np.random.RandomState(13)
    a, b = rng.randn(2 * CHUNK + 10).astype(np.float32), rng.randn(100).astype(np.float32)
    clean = _run([_cuda(a), _cuda(b)])
    a[CHUNK + 3] = np.nan
    got = _run([_cuda(a), _cuda(b)])
    assert np.isnan(got).tolist() == [False, True, False, False]
    keep = [0, 2, 3]
    assert got[keep].tobytes() == clean[keep].tobytes()


def test_sumsq_past_two_to_the_31_elements():
    """One bf16 tensor of 2^31 + CHUNK + 3 elements: element indices and byte offsets beyond 32 bits.  Zeros but for the last chunks."""
    import torch
    n = 2 ** 31 + CHUNK + 3
    t = torch.zeros((n,), dtype=torch.bfloat16, device="cuda")
    t[2 ** 31 - 1] = 2.0
    t[2 ** 31] = 3.0
    t[n - 1] = 4.0
    got = _run([t])
    assert got.shape == (2 ** 31 // CHUNK + 2,)
    assert got[-3:].tolist() == [4.0, 9.0, 16.0] and float(got[:-3].max()) == 0.0 and float(got.astype(np.float64).sum()) == 29.0


def test_refusals_happen_before_anything_is_launched():
    import torch
    nat = _nat()
    lib = nat.load()
    stream = nat.current_stream_ptr(torch.device("cuda", torch.cuda.current_device()))
    t = _cuda(np.ones(100, np.float32))
    out = torch.full((4,), float("nan"), dtype=torch.float32, device="cuda")
    sentinel = out.cpu().numpy().tobytes()
    ptrs, counts = (ctypes.c_void_p * 2)(t.data_ptr(), t.data_ptr()), (ctypes.c_longlong * 2)(100, 100)
    po = ctypes.c_void_p(out.data_ptr())
    call = lambda n, p, c, dtype, o, n_out: lib.ssdhip_sumsq_partials(n, p, c, dtype, o, n_out, stream)
    assert call(2, ptrs, counts, nat.SUMSQ_F32, po, 2) == 0                  # (the accepted form of the calls below)
    torch.cuda.synchronize()
    assert out.cpu().numpy()[:2].tolist() == [100.0, 100.0]
    out.fill_(float("nan"))
    bad = [call(2, ptrs, counts, 2, po, 2),                                   # unknown dtype flag
           call(2, ptrs, counts, -1, po, 2),
           call(-1, ptrs, counts, nat.SUMSQ_F32, po, 2),                      # negative table length
           call(2, ptrs, (ctypes.c_longlong * 2)(100, -1), nat.SUMSQ_F32, po, 1),   # negative element count
           call(2, ptrs, counts, nat.SUMSQ_F32, po, 3),                       # not the table's chunk count
           call(2, ptrs, counts, nat.SUMSQ_F32, po, -2),
           call(2, (ctypes.c_void_p * 2)(t.data_ptr(), None), counts, nat.SUMSQ_F32, po, 2),       # a null tensor
           call(2, (ctypes.c_void_p * 2)(t.data_ptr(), t.data_ptr() + 2), counts, nat.SUMSQ_F32, po, 2),   # float32 at a 2-byte offset
           call(2, (ctypes.c_void_p * 2)(t.data_ptr(), t.data_ptr() + 1), counts, nat.SUMSQ_BF16, po, 2),  # bf16 at an odd address
           call(2, ptrs, counts, nat.SUMSQ_F32, None, 2),                     # no output
           call(2, None, counts, nat.SUMSQ_F32, po, 2)]
    torch.cuda.synchronize()
    assert bad == [-1] * len(bad) and out.cpu().numpy().tobytes() == sentinel
    # the meter
    whole, block, at = _block(fill=0xAB)
    before = whole.cpu().numpy().tobytes()
    loss = _cuda(np.ones(3, np.float32))
    pl, ps = ctypes.c_void_p(loss.data_ptr()), ctypes.c_void_p(block.data_ptr())
    upd = lambda l, b, p, n, s: lib.ssdhip_fit_meter_update(l, b, p, n, 0.5, s, stream)
    bad = [upd(pl, 3, None, 0, None), upd(pl, 3, None, 0, ctypes.c_void_p(block.data_ptr() + 8)),   # null / misaligned state
           upd(pl, 0, None, 0, ps), upd(pl, -3, None, 0, ps),                  # B <= 0
           upd(pl, 3, None, -1, ps), upd(pl, 3, None, 2, ps),                  # negative count; partials promised but absent
           upd(None, 3, None, 0, ps),
           lib.ssdhip_fit_meter_reset(None, stream), lib.ssdhip_fit_meter_reset(ctypes.c_void_p(block.data_ptr() + 4), stream)]
    torch.cuda.synchronize()
    assert bad == [-1] * len(bad) and whole.cpu().numpy().tobytes() == before
    assert lib.ssdhip_fit_meter_state_bytes() == 48
