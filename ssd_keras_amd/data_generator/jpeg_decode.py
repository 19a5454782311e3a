"""Baseline JPEG decoding of a batch of files on the device (a `DataGenerator` whose `decode` is 'device'; not in the reference, whose images are
decoded by PIL one file at a time).

`plan_jpeg` parses a file's markers on the host and returns a `JpegPlan` for the subset the kernels decode, None for everything
else; `decode_jpeg_batch` uploads the plans of a batch as ONE descriptor buffer (image headers, segment table, quantisation tables,
Huffman tables in look-up form, the compressed bytes) and runs csrc/ssdhip_jpeg.hip on it: Huffman decoding with one lane per
(image, restart segment), dequantisation + libjpeg's "islow" IDCT per block, "fancy" chroma upsampling and the fixed-point
YCbCr -> RGB conversion per pixel.  Every step is integer arithmetic, and the result equals `np.array(PIL.Image.open(f))` bit for bit.

The subset: 8-bit, Huffman-coded, sequential (SOF0 / SOF1), ONE scan; one component (-> (H, W)) or three interleaved components
(-> (H, W, 3)) with luma sampling 1x1, 2x1 or 2x2 over 1x1 chroma; colour space plainly YCbCr (a JFIF marker, or an Adobe marker
with transform 1, or neither and component ids 1, 2, 3); an optional restart interval whose markers are all there, in order.  None
for progressive, lossless, arithmetic-coded and 12-bit files, CMYK / YCCK, Adobe transform 0 or other component ids, other sampling
factors, several scans, a table the scan names but the file lacks, a segment length that leaves the file -- and for anything that is
no JPEG.  PIL decodes those as before, and it decodes every image whose device status word is set (truncated or corrupt entropy data,
csrc/ssdhip_jpeg_entropy.h): PIL's own result, or its exception, is what the caller gets.

A file without restart markers is one segment, so one lane decodes it however large the batch is.  Training reads the same files every
epoch: with a `JpegIndex` (`decode_jpeg_batch(..., index=...)`) such a file is decoded sequentially ONCE while the device records
where every MCU row starts (byte, bit, DC predictors: 32 bytes per row), and from its second sight on with one lane per MCU row.  Each
lane checks that it ends exactly on the next row's entry, so a wrong or stale index cannot give other pixels: the file's status word is
set, its entry is dropped and it is decoded again by the recording route in the same call.
"""
from __future__ import annotations

import ctypes
import hashlib

import numpy as np

from .. import _native as nat

# How often each thing happened since import (tests and tools read and reset these): images the device decoded, images PIL decoded
# inside decode_jpeg_batch, device images copied back to the host by `to_host`; of the device's images, those decoded through their
# index entry ("indexed") and those whose entry was recorded by the call ("recorded").
COUNTERS = {"device": 0, "host": 0, "downloaded": 0, "indexed": 0, "recorded": 0}

ST_INDEX = 32                   # SSDHIP_JPEG_ST_INDEX (csrc/ssdhip_jpeg_entropy.h)
ENTRY_WORDS = 8                 # struct ssdhip_jpeg_entry: image, byte, bit, first_mcu, n_mcus, pred0, pred1, pred2

CHUNK = 256                     # files per call when a whole dataset is decoded (DataGenerator(load_images_into_memory=True))
_MAX_BYTES = 1 << 30            # compressed bytes / blocks per call: offsets are 32-bit ints on the device
_MAX_BLOCKS = 1 << 22

_NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47,
                     55, 62, 63], dtype=np.int64)


class JpegPlan:
    """What the kernels need to know about one file.  height, width, ncomp (1 or 3), hs, vs (luma sampling), mcux, mcuy (MCU grid),
    restart_interval (0: none), qt_ids / dc_ids / ac_ids (per component: the file's table numbers), qtables / dc_tables / ac_tables
    (per component: uint16[64] in natural order; (counts bytes[16], symbols bytes)), segments ([(begin, end)] byte ranges of the
    entropy-coded segments in the file, restart markers excluded), has_eoi (False: the file ends inside or right behind its scan;
    the device result of such a file is never used)."""

    __slots__ = ("height", "width", "ncomp", "hs", "vs", "mcux", "mcuy", "restart_interval", "qt_ids", "dc_ids", "ac_ids", "qtables",
                 "dc_tables", "ac_tables", "_segments", "has_eoi")

    @property
    def segments(self):
        return [(int(b), int(e)) for b, e in self._segments]

    @segments.setter
    def segments(self, ranges):
        self._segments = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)

    @property
    def shape(self):
        return (self.height, self.width) if self.ncomp == 1 else (self.height, self.width, 3)

    @property
    def nblocks(self):
        return self.mcux * self.mcuy * (self.hs * self.vs + (2 if self.ncomp == 3 else 0))

    @property
    def interval(self):
        """MCUs per segment."""
        return self.restart_interval if self.restart_interval else self.mcux * self.mcuy


def _huffman_ok(counts, symbols, dc):
    """libjpeg's own table checks: the code lengths form a prefix code, and a DC table holds categories 0..15 only."""
    code = 0
    for length, n in enumerate(counts, start=1):
        code += n
        if code > (1 << length):
            return False
        code <<= 1
    return not dc or all(s <= 15 for s in symbols)


def plan_jpeg(data):
    """bytes of a file -> JpegPlan, or None if PIL has to decode it (module docstring).  Never raises for any bytes."""
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        return None
    qtables, huff, frame, interval, jfif, adobe = {}, {}, None, 0, False, None
    pos = 2
    while True:
        if pos + 4 > n or data[pos] != 0xFF:
            return None
        while pos < n and data[pos] == 0xFF:            # fill bytes
            pos += 1
        if pos >= n:
            return None
        marker = data[pos]
        pos += 1
        if pos + 2 > n:
            return None
        length = (data[pos] << 8) | data[pos + 1]
        if marker in (0xD8, 0xD9, 0x01, 0x00) or 0xD0 <= marker <= 0xD7 or length < 2 or pos + length > n:
            return None
        body = data[pos + 2:pos + length]
        pos += length
        if marker == 0xE0:
            jfif = jfif or body[:5] == b"JFIF\0"
        elif marker == 0xEE:
            if body[:5] == b"Adobe" and len(body) >= 12:
                adobe = body[11]
        elif 0xE0 <= marker <= 0xEF or marker == 0xFE:
            pass
        elif marker == 0xDB:
            k = 0
            while k < len(body):
                pq, tq = body[k] >> 4, body[k] & 15
                size = 64 if pq == 0 else 128
                if pq > 1 or tq > 3 or k + 1 + size > len(body):
                    return None
                raw = np.frombuffer(body, dtype=np.uint8 if pq == 0 else ">u2", count=64, offset=k + 1).astype(np.int64)
                if raw.max() > 32767:                   # libjpeg keeps the IDCT's multipliers as 16-bit signed values
                    return None
                table = np.zeros(64, dtype=np.uint16)
                table[_NATURAL] = raw
                qtables[tq] = table
                k += 1 + size
        elif marker == 0xC4:
            k = 0
            while k < len(body):
                tc, th = body[k] >> 4, body[k] & 15
                if tc > 1 or th > 3 or k + 17 > len(body):
                    return None
                counts = bytes(body[k + 1:k + 17])
                total = sum(counts)
                if total > 256 or k + 17 + total > len(body):
                    return None
                symbols = bytes(body[k + 17:k + 17 + total])
                if not _huffman_ok(counts, symbols, tc == 0):
                    return None
                huff[(tc, th)] = (counts, symbols)
                k += 17 + total
        elif marker in (0xC0, 0xC1):
            if frame is not None or len(body) < 6:
                return None
            precision, height, width, nc = body[0], (body[1] << 8) | body[2], (body[3] << 8) | body[4], body[5]
            if precision != 8 or height == 0 or width == 0 or nc not in (1, 3) or len(body) != 6 + 3 * nc:
                return None
            frame = (height, width, [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(nc)])
        elif marker == 0xDD:
            if len(body) != 2:
                return None
            interval = (body[0] << 8) | body[1]
        elif marker == 0xDA:
            break
        else:                                           # SOF2.. (progressive, lossless, arithmetic), DAC, DNL, DHP, EXP, reserved
            return None

    if frame is None:
        return None
    height, width, comps = frame
    nc = len(comps)
    if len(body) != 4 + 2 * nc or body[0] != nc:        # one scan with every component (interleaved)
        return None
    scan = [(body[1 + 2 * c], body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(nc)]
    if [s[0] for s in scan] != [c[0] for c in comps] or tuple(body[1 + 2 * nc:4 + 2 * nc]) != (0, 63, 0):
        return None
    if nc == 1:
        if (comps[0][1], comps[0][2]) != (1, 1):
            return None
        hs = vs = 1
    else:
        hs, vs = comps[0][1], comps[0][2]
        if (hs, vs) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            return None
        ids = tuple(c[0] for c in comps)
        if not jfif and (adobe != 1 if adobe is not None else ids != (1, 2, 3)):
            return None
    if any(c[3] not in qtables for c in comps) or any((0, s[1]) not in huff or (1, s[2]) not in huff for s in scan):
        return None

    plan = JpegPlan()
    plan.height, plan.width, plan.ncomp, plan.hs, plan.vs = height, width, nc, hs, vs
    plan.mcux, plan.mcuy = -(-width // (8 * hs)), -(-height // (8 * vs))
    plan.restart_interval = interval
    plan.qt_ids, plan.dc_ids, plan.ac_ids = [c[3] for c in comps], [s[1] for s in scan], [s[2] for s in scan]
    plan.qtables = [qtables[c[3]] for c in comps]
    plan.dc_tables, plan.ac_tables = [huff[(0, s[1])] for s in scan], [huff[(1, s[2])] for s in scan]

    # the scan's bytes: up to the first marker that is neither a stuffed FF nor a restart marker (or the end of the file)
    arr = np.frombuffer(data, dtype=np.uint8)
    ff = pos + np.flatnonzero(arr[pos:n - 1] == 0xFF)
    follow = arr[ff + 1]
    is_restart = (follow >= 0xD0) & (follow <= 0xD7)
    others = ff[(follow != 0) & ~is_restart]
    scan_end = int(others[0]) if len(others) else n
    restarts = ff[is_restart & (ff < scan_end)]
    k = scan_end
    while k < n and data[k] == 0xFF:
        k += 1
    plan.has_eoi = scan_end < n and k < n and data[k] == 0xD9
    if scan_end < n and not plan.has_eoi and k < n:     # another scan, or tables behind the scan: not this subset
        return None
    total = plan.mcux * plan.mcuy
    expected = (-(-total // interval) - 1) if interval else 0
    if interval:
        if len(restarts) != expected or not np.array_equal(arr[restarts + 1], 0xD0 + (np.arange(expected) & 7)):
            return None
    elif len(restarts):
        return None
    plan._segments = np.stack([np.concatenate([[pos], restarts + 2]), np.concatenate([restarts, [scan_end]])], axis=1).astype(np.int64)
    return plan


# ---- the descriptor buffer ------------------------------------------------------------------------------------------------------------
_huff_cache = {}
_layout_checked = False


def huffman_lookup(counts, symbols):
    """A DHT table -> the SSDHIP_JPEG_HUFF_BYTES bytes of struct ssdhip_jpeg_huff (csrc/ssdhip_jpeg_entropy.h)."""
    key = (counts, symbols)
    got = _huff_cache.get(key)
    if got is not None:
        return got
    look = np.zeros(256, dtype=np.uint16)
    maxcode = np.full(18, -1, dtype=np.int32)
    valoff = np.zeros(18, dtype=np.int32)
    vals = np.zeros(256, dtype=np.uint8)
    vals[:len(symbols)] = np.frombuffer(symbols, dtype=np.uint8)
    code, k = 0, 0
    for length in range(1, 17):
        cnt = counts[length - 1]
        if cnt:
            valoff[length] = k - code
            if length <= 8:
                span = 1 << (8 - length)
                for j in range(cnt):
                    look[(code + j) * span:(code + j + 1) * span] = (length << 8) | symbols[k + j]
            k += cnt
            code += cnt
            maxcode[length] = code - 1
        code <<= 1
    maxcode[17] = 0xFFFFF
    table = np.concatenate([look.view(np.uint8), maxcode.view(np.uint8), valoff.view(np.uint8), vals])
    if len(_huff_cache) > 512:
        _huff_cache.clear()
    _huff_cache[key] = table
    return table


def _align(v, a=16):
    return -(-v // a) * a


RECORD = "record"                # pack_plans(index_rows=[...]): decode this image sequentially and record its entries


def pack_plans(plans, datas, align=256, index_rows=None):
    """The descriptor buffer of a batch (plans[i] of datas[i]) as the device reads it: (host uint8 array, dict of the launch's
    arguments, [(out_offset, shape)] per image).  Parts are 16-byte aligned; the status words are the zeros at its end.

    `index_rows` (ssdhip_jpeg_decode_batch_indexed; None: the buffer and the arguments are exactly those without it): per image None
    (the per-segment path), RECORD, or the image's int32 (rows, 8) entries as a `JpegIndex` keeps them (`byte` counted from the start
    of the scan's bytes).  Behind the status words the buffer then holds one mode word per image and the entry table (struct
    ssdhip_jpeg_entry, `image` and `byte` set for this batch), and the arguments gain off_modes, off_entries, n_entries, ckpt_entries,
    record_segments and ckpt_base (per image: its first row in the checkpoint buffer, or None)."""
    n = len(plans)
    images = np.zeros((n, 24), dtype=np.int32)
    qt_index, qt_list, huff_index, huff_list = {}, [], {}, []
    segments, chunks, outs = [], [], []
    data_pos = block_pos = out_pos = 0
    modes, entries, ckpt_base, ckpt_pos, n_seg = np.zeros(n, dtype=np.int32), [], [None] * n, 0, 0

    def huff_id(t):
        i = huff_index.get(t)
        if i is None:
            i = huff_index[t] = len(huff_list)
            huff_list.append(huffman_lookup(*t))
        return i

    for i, (p, d) in enumerate(zip(plans, datas)):
        row = images[i]
        row[:8] = (p.height, p.width, p.ncomp, p.hs, p.vs, p.mcux, p.mcuy, p.interval)
        for c in range(p.ncomp):
            key = p.qtables[c].tobytes()
            q = qt_index.get(key)
            if q is None:
                q = qt_index[key] = len(qt_list)
                qt_list.append(p.qtables[c])
            row[8 + c], row[11 + c], row[14 + c] = q, huff_id(p.dc_tables[c]), huff_id(p.ac_tables[c])
        row[17], row[20] = block_pos, p.nblocks
        images[i:i + 1].view(np.int64)[0, 9] = out_pos
        seg = p._segments
        if index_rows is not None and index_rows[i] is not None:
            if isinstance(index_rows[i], str):
                modes[i] = (ckpt_pos << 2) | 2
                ckpt_base[i] = ckpt_pos
                ckpt_pos += p.mcuy
            else:
                rows = np.array(index_rows[i], dtype=np.int64).reshape(-1, ENTRY_WORDS)
                rows[:, 0] = i
                rows[:, 1] += data_pos
                entries.append(np.clip(rows, -2 ** 31, 2 ** 31 - 1))
                modes[i] = (n_seg << 2) | 1
        n_seg += len(seg)
        first, last = int(seg[0, 0]), int(seg[-1, 1])
        rows = np.empty((len(seg), 4), dtype=np.int64)
        rows[:, 0], rows[:, 1:3], rows[:, 3] = i, seg + (data_pos - first), np.arange(len(seg)) * p.interval
        segments.append(rows)
        chunks.append(d[first:last])
        data_pos += last - first
        block_pos += p.nblocks
        outs.append((out_pos, p.shape))
        out_pos += _align(p.height * p.width * p.ncomp, align)
    segments = np.concatenate(segments).astype(np.int32)
    qt = np.stack(qt_list).astype(np.uint16)
    huff = np.stack(huff_list)
    off_images = 0
    off_segments = _align(images.nbytes)
    off_qt = off_segments + _align(segments.nbytes)
    off_huff = off_qt + _align(qt.nbytes)
    off_data = off_huff + _align(huff.nbytes)
    off_status = off_data + _align(data_pos)
    size = off_status + _align(4 * n)
    if index_rows is not None:
        entries = np.concatenate(entries).astype(np.int32) if entries else np.zeros((0, ENTRY_WORDS), dtype=np.int32)
        off_modes = size
        off_entries = off_modes + _align(4 * n)
        size = off_entries + _align(entries.nbytes)
    host = np.zeros(size, dtype=np.uint8)
    host[off_images:off_images + images.nbytes] = images.view(np.uint8).ravel()
    host[off_segments:off_segments + segments.nbytes] = segments.view(np.uint8).ravel()
    host[off_qt:off_qt + qt.nbytes] = qt.view(np.uint8).ravel()
    host[off_huff:off_huff + huff.nbytes] = huff.ravel()
    host[off_data:off_data + data_pos] = np.frombuffer(b"".join(chunks), dtype=np.uint8)
    args = dict(n_images=n, n_segments=len(segments), n_qt=len(qt_list), n_huff=len(huff_list), off_images=off_images,
                off_segments=off_segments, off_qt=off_qt, off_huff=off_huff, off_data=off_data, data_bytes=data_pos, off_status=off_status,
                max_blocks=max(p.nblocks for p in plans), max_pixels=max(p.height * p.width for p in plans), total_blocks=block_pos,
                out_bytes=max(out_pos, 1))
    if index_rows is not None:
        host[off_modes:off_modes + 4 * n] = modes.view(np.uint8)
        host[off_entries:off_entries + entries.nbytes] = entries.view(np.uint8).ravel()
        indexed = (modes & 3) == 1
        args.update(off_modes=off_modes, off_entries=off_entries, n_entries=len(entries), ckpt_entries=ckpt_pos, ckpt_base=ckpt_base,
                    record_segments=int(sum(len(p._segments) for p, m in zip(plans, indexed) if not m)))
    return host, args, outs


def lanes_per_wave(n_segments):
    """Segments per 64-lane workgroup of the entropy launch.  A lane pays for the branches of every lane it shares its wave with, so
    few segments are spread one per wave over the chip's 256 CUs x 4 SIMDs x 8 wave slots, and only more than those share waves."""
    return int(min(64, max(1, -(-n_segments // 8192))))


def _check_layout():
    global _layout_checked
    if not _layout_checked:
        words = (ctypes.c_int * 4)()
        nat.check(nat.load().ssdhip_jpeg_layout(words), "ssdhip_jpeg_layout")
        from ._image_ops import RAGGED_ALIGN
        if list(words) != [24, 4, 912, RAGGED_ALIGN]:
            raise nat.SsdHipError("libssdhip.so's JPEG descriptors are not this module's: rebuild it")
        words = (ctypes.c_int * 2)()
        nat.check(nat.load().ssdhip_jpeg_entry_layout(words), "ssdhip_jpeg_entry_layout")
        if list(words) != [ENTRY_WORDS, ST_INDEX]:
            raise nat.SsdHipError("libssdhip.so's JPEG index entries are not this module's: rebuild it")
        _layout_checked = True


def _load_image(source):
    """The host decoder: `_load_image` of the generator for a file name; the same call on the bytes otherwise."""
    from .object_detection_2d_data_generator import _load_image as load
    if isinstance(source, (bytes, bytearray, memoryview)):
        import io
        return load(io.BytesIO(source))
    return load(source)


def _read(source):
    if isinstance(source, (bytes, bytearray, memoryview)):
        return bytes(source)
    with open(source, "rb") as f:
        return f.read()


def decode_planned(plans, datas, device=None, stages=7, events=None, index_rows=None):
    """The device part of `decode_jpeg_batch` for files that all have a plan: -> (list of CUDA uint8 views into one output buffer,
    status (n,) int32 NumPy array).  `stages`: ssdhip_jpeg_decode_batch's bit mask; `events`: a callable that is called between the
    upload and each stage's launch (tools/time_jpeg_decode.py records device events there).  With `index_rows` (`pack_plans`) the
    call is ssdhip_jpeg_decode_batch_indexed and returns a third value: per image None, or for a RECORD image whose status is 0 its
    recorded int32 (rows, 8) entries in `JpegIndex` form."""
    import torch
    _check_layout()
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    from ._image_ops import RAGGED_ALIGN
    host, a, outs = pack_plans(plans, datas, RAGGED_ALIGN, index_rows=index_rows)
    desc = torch.from_numpy(host).to(device)
    out = torch.empty((a["out_bytes"],), dtype=torch.uint8, device=device)
    coef = nat.workspaces.get(device, "jpeg_coef", a["total_blocks"] * 128)
    planes = nat.workspaces.get(device, "jpeg_planes", a["total_blocks"] * 64)
    ckpt = None
    if index_rows is not None and a["ckpt_entries"]:
        ckpt = torch.empty((a["ckpt_entries"], ENTRY_WORDS), dtype=torch.int32, device=device)
    for stage in (1, 2, 4):
        if events is not None:
            events()
        if not stages & stage:
            continue
        if index_rows is None:
            nat.launch("ssdhip_jpeg_decode_batch", device, nat._ptr(desc), desc.numel(), a["n_images"], a["n_segments"], a["n_qt"],
                       a["n_huff"], a["off_images"], a["off_segments"], a["off_qt"], a["off_huff"], a["off_data"], a["data_bytes"],
                       a["off_status"], a["max_blocks"], a["max_pixels"], a["total_blocks"], lanes_per_wave(a["n_segments"]), stage,
                       nat._ptr(coef), nat._ptr(planes), nat._ptr(out), a["out_bytes"])
        else:
            nat.launch("ssdhip_jpeg_decode_batch_indexed", device, nat._ptr(desc), desc.numel(), a["n_images"], a["n_segments"], a["n_qt"],
                       a["n_huff"], a["off_images"], a["off_segments"], a["off_qt"], a["off_huff"], a["off_data"], a["data_bytes"],
                       a["off_status"], a["off_entries"], a["n_entries"], a["off_modes"], nat._ptr(ckpt), a["ckpt_entries"],
                       a["record_segments"], a["max_blocks"], a["max_pixels"], a["total_blocks"], lanes_per_wave(a["n_entries"]),
                       lanes_per_wave(a["record_segments"]), stage, nat._ptr(coef), nat._ptr(planes), nat._ptr(out), a["out_bytes"])
    if events is not None:
        events()
    status = desc[a["off_status"]:a["off_status"] + 4 * a["n_images"]].cpu().numpy().view(np.int32)
    views = []
    for o, shape in outs:
        views.append(out[o:o + int(np.prod(shape))].view(*shape))
    if index_rows is None:
        return views, status
    recorded = [None] * len(plans)
    if ckpt is not None and stages & 1:
        rows = ckpt.cpu().numpy()
        seg_begin = np.frombuffer(host, dtype=np.int32, count=4 * a["n_segments"], offset=a["off_segments"]).reshape(-1, 4)
        begin_of = {int(r[0]): int(r[1]) for r in seg_begin[::-1]}           # image -> begin of its first segment
        for i, (p, base) in enumerate(zip(plans, a["ckpt_base"])):
            if base is not None and status[i] == 0:
                mine = rows[base:base + p.mcuy].copy()
                mine[:, 1] -= begin_of[i]
                mine[:, 0] = 0
                recorded[i] = mine
    return views, status, recorded


class JpegIndex:
    """Entry points of files without restart markers: key -> int32 (MCU rows, 8) array of struct ssdhip_jpeg_entry rows (`image` 0,
    `byte` counted from the first byte of the scan's entropy-coded data).  The key of a file NAME is the name plus the file's length,
    the key of bytes their digest (`key`).  An entry is only ever a hint: the device verifies it while it decodes (module
    docstring), so a file that changed under its name, or an index loaded from elsewhere, costs one recording decode and nothing
    else.  At most `max_files` entries are kept (the oldest go first); about 32 bytes per 8 or 16 image rows each."""

    def __init__(self, max_files=1 << 20):
        self.max_files = int(max_files)
        self._rows = {}

    @staticmethod
    def key(source, data):
        """The key of `source` (a file name, or bytes) whose content is `data`.  The digest of bytes covers their length, their
        first 4 KiB (the headers and the start of the scan) and their last 4 KiB: enough to tell files apart at a fixed cost, and
        an entry that is not the file's is rejected on the device anyway."""
        if isinstance(source, (bytes, bytearray, memoryview)):
            h = hashlib.blake2b(len(data).to_bytes(8, "little"), digest_size=16)
            h.update(data[:4096])
            h.update(data[-4096:])
            return "d:" + h.hexdigest()
        return "f:%d:%s" % (len(data), source)

    def __len__(self):
        return len(self._rows)

    def __contains__(self, key):
        return key in self._rows

    def __getitem__(self, key):
        return self._rows[key]

    def get(self, key):
        return self._rows.get(key)

    def __setitem__(self, key, rows):
        rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, ENTRY_WORDS)
        self._rows.pop(key, None)
        self._rows[key] = rows
        while len(self._rows) > max(self.max_files, 0):
            del self._rows[next(iter(self._rows))]

    def pop(self, key, default=None):
        return self._rows.pop(key, default)

    def keys(self):
        return list(self._rows)

    def clear(self):
        self._rows.clear()

    def save(self, path):
        """One .npz of plain arrays: the keys, the row count of each, all rows."""
        keys = list(self._rows)
        counts = np.array([len(self._rows[k]) for k in keys], dtype=np.int64)
        rows = np.concatenate([self._rows[k] for k in keys]) if keys else np.zeros((0, ENTRY_WORDS), dtype=np.int32)
        with open(path, "wb") as f:
            np.savez(f, keys=np.array(keys, dtype=np.str_), counts=counts, rows=rows.astype(np.int32))

    @classmethod
    def load(cls, path, max_files=1 << 20):
        self = cls(max_files)
        with np.load(path, allow_pickle=False) as z:
            keys, counts, rows = [str(k) for k in z["keys"]], z["counts"].astype(np.int64), z["rows"].astype(np.int32)
        if rows.ndim != 2 or rows.shape[1] != ENTRY_WORDS or len(keys) != len(counts) or (counts < 0).any() or counts.sum() != len(rows):
            raise ValueError("%s is no JpegIndex file" % path)
        ends = np.cumsum(counts)
        for k, n, e in zip(keys, counts, ends):
            self[k] = rows[e - n:e].copy()
        return self


def _uses_index(plan):
    """The index is for planned files without a restart interval and with at least two MCU rows (a lane per row is the gain); a
    file that ends inside its scan is PIL's whatever the device makes of it."""
    return plan.restart_interval == 0 and plan.mcuy >= 2 and plan.has_eoi


def decode_jpeg_batch(sources, device=None, index=None):
    """File names or bytes -> one entry per source, in order: a CUDA uint8 tensor (H, W) / (H, W, 3) for every file the device
    decoded -- views into ONE output buffer, each on a RAGGED_ALIGN boundary, so `_image_ops.pack_ragged` copies them into place on
    the device --, and for a file without a plan, or one whose device status is non-zero, the NumPy array `_load_image` returns.  An
    exception `_load_image` raises is raised unchanged.  The batch's descriptors go up as ONE host buffer in one copy; the status
    words come back in one.  (A batch of more than 1 GiB of compressed bytes or 2^22 blocks is decoded as two; each half then has
    its own output buffer.)

    `index`: a `JpegIndex`, used and filled in place (None: no file is indexed and the call is ssdhip_jpeg_decode_batch).  A file
    without restart markers that has an entry is decoded through it; one that has none is decoded sequentially and its entry
    recorded.  A file whose indexed decode reports any status loses its entry and is decoded again by the recording route -- all such
    files of the call in ONE second launch, whose views lie in a second output buffer -- and goes to PIL only if that fails too."""
    sources = list(sources)
    datas = [_read(s) for s in sources]
    plans = [plan_jpeg(d) for d in datas]
    idx = [i for i, p in enumerate(plans) if p is not None]
    if len(idx) > 1 and (sum(len(datas[i]) for i in idx) > _MAX_BYTES or sum(plans[i].nblocks for i in idx) > _MAX_BLOCKS):
        half = len(sources) // 2
        return decode_jpeg_batch(sources[:half], device, index) + decode_jpeg_batch(sources[half:], device, index)
    results = [None] * len(sources)
    if idx and index is None:
        views, status = decode_planned([plans[i] for i in idx], [datas[i] for i in idx], device)
        for i, v, st in zip(idx, views, status):
            if st == 0 and plans[i].has_eoi:
                results[i] = v
                COUNTERS["device"] += 1
    elif idx:
        keys = {i: JpegIndex.key(sources[i], datas[i]) for i in idx if _uses_index(plans[i])}
        rows = []
        for i in idx:
            known = index.get(keys[i]) if i in keys else None
            if known is not None and len(known) != plans[i].mcuy:        # not this file's: no need to ask the device
                index.pop(keys[i])
                known = None
            rows.append(None if i not in keys else (RECORD if known is None else known))
        views, status, recorded = decode_planned([plans[i] for i in idx], [datas[i] for i in idx], device, index_rows=rows)
        again = []
        for i, v, st, r, rec in zip(idx, views, status, rows, recorded):
            if st == 0 and plans[i].has_eoi:
                results[i] = v
                COUNTERS["device"] += 1
                if rec is not None:
                    index[keys[i]] = rec
                    COUNTERS["recorded"] += 1
                elif r is not None:
                    COUNTERS["indexed"] += 1
            elif r is not None and not isinstance(r, str):               # the index was rejected (or the file is damaged)
                index.pop(keys[i])
                again.append(i)
        if again:
            views, status, recorded = decode_planned([plans[i] for i in again], [datas[i] for i in again], device,
                                                     index_rows=[RECORD] * len(again))
            for i, v, st, rec in zip(again, views, status, recorded):
                if st == 0:
                    results[i] = v
                    index[keys[i]] = rec
                    COUNTERS["device"] += 1
                    COUNTERS["recorded"] += 1
    for i, s in enumerate(sources):
        if results[i] is None:
            results[i] = _load_image(s)
            COUNTERS["host"] += 1
    return results


def to_host(images):
    """The images of a `decode_jpeg_batch` result as NumPy arrays (device members are downloaded and counted)."""
    out = []
    for im in images:
        if isinstance(im, np.ndarray):
            out.append(im)
        else:
            COUNTERS["downloaded"] += 1
            out.append(im.cpu().numpy())
    return out
