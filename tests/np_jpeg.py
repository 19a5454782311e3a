"""Baseline JPEG decoding restated in NumPy / plain Python, the way libjpeg-turbo performs it with PIL's settings: sequential Huffman
entropy decoding, dequantisation inside the jidctint "islow" IDCT (13-bit constants, PASS1_BITS 2, range limit), "fancy" h2v1 / h2v2
chroma upsampling and the 16-bit fixed-point YCbCr -> RGB conversion.  It has its own marker parser (the files the tests make: one
interleaved scan, 8-bit tables) so that it checks `jpeg_decode.plan_jpeg` too, and its entropy loop carries the bounds and status
rules of csrc/ssdhip_jpeg_entropy.h: reads stop at the segment's end or at a marker, consuming made-up bits is TRUNCATED, a code no
table holds is BADCODE, a run past coefficient 63 is RUN, and the segment stops at the first of them."""
import numpy as np

ST_TRUNCATED, ST_BADCODE, ST_RUN = 1, 2, 4

NATURAL = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47,
           55, 62, 63]


class Parsed:
    pass


def parse(data):
    """Markers of a baseline file -> Parsed (height, width, comps [(id, h, v, tq)], scan [(td, ta)], qt {id: int array in natural
    order}, huff {(class, id): (counts, symbols)}, interval, segments [(begin, end)])."""
    assert data[:2] == b"\xff\xd8"
    p = Parsed()
    p.qt, p.huff, p.interval = {}, {}, 0
    pos = 2
    while True:
        assert data[pos] == 0xFF
        marker = data[pos + 1]
        length = (data[pos + 2] << 8) | data[pos + 3]
        body = data[pos + 4:pos + 2 + length]
        pos += 2 + length
        if marker == 0xDB:
            k = 0
            while k < len(body):
                pq, tq = body[k] >> 4, body[k] & 15
                if pq == 0:
                    raw = list(body[k + 1:k + 65])
                    k += 65
                else:
                    raw = [(body[k + 1 + 2 * j] << 8) | body[k + 2 + 2 * j] for j in range(64)]
                    k += 129
                table = np.zeros(64, dtype=np.int64)
                for j in range(64):
                    table[NATURAL[j]] = raw[j]
                p.qt[tq] = table
        elif marker == 0xC4:
            k = 0
            while k < len(body):
                counts = list(body[k + 1:k + 17])
                total = sum(counts)
                p.huff[(body[k] >> 4, body[k] & 15)] = (counts, list(body[k + 17:k + 17 + total]))
                k += 17 + total
        elif marker in (0xC0, 0xC1):
            assert body[0] == 8
            p.height, p.width = (body[1] << 8) | body[2], (body[3] << 8) | body[4]
            p.comps = [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(body[5])]
        elif marker == 0xDD:
            p.interval = (body[0] << 8) | body[1]
        elif marker == 0xDA:
            assert body[0] == len(p.comps)
            p.scan = [(body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(body[0])]
            break
        else:
            assert 0xE0 <= marker <= 0xEF or marker == 0xFE, hex(marker)
    # the entropy-coded segments: split at RSTn, end at the first other marker (or the end of the bytes)
    p.segments, begin, k, n = [], pos, pos, len(data)
    while True:
        if k >= n - 1:
            p.segments.append((begin, n))
            break
        if data[k] == 0xFF and data[k + 1] != 0:
            if 0xD0 <= data[k + 1] <= 0xD7:
                p.segments.append((begin, k))
                begin = k = k + 2
                continue
            p.segments.append((begin, k))
            break
        k += 1
    return p


def geometry(p):
    """(hs, vs, mcux, mcuy, blocks per component [(grid height, grid width)])."""
    hs, vs = (p.comps[0][1], p.comps[0][2]) if len(p.comps) == 3 else (1, 1)
    mcux, mcuy = -(-p.width // (8 * hs)), -(-p.height // (8 * vs))
    grids = [(mcuy * vs, mcux * hs)] + [(mcuy, mcux)] * (len(p.comps) - 1)
    return hs, vs, mcux, mcuy, grids


def _decode_table(counts, symbols):
    """16-bit look-up: table[first 16 bits] = (length, symbol), or None for bits that start no code."""
    table = [None] * 65536
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            lo = code << (16 - length)
            table[lo:lo + (1 << (16 - length))] = [(length, symbols[k])] * (1 << (16 - length))
            code += 1
            k += 1
        code <<= 1
    return table


_tables = {}


def _table(t):
    key = (tuple(t[0]), tuple(t[1]))
    if key not in _tables:
        if len(_tables) > 64:
            _tables.clear()
        _tables[key] = _decode_table(*t)
    return _tables[key]


def _extend(v, s):
    return 0 if s == 0 else (v - (1 << s) + 1 if v < (1 << (s - 1)) else v)


def entropy(data, p):
    """Coefficients int16 [blocks][64] (natural order; the components' block grids one after the other) and the status (the OR over
    the segments of the status that stopped each).  Blocks a stopped segment did not reach stay as they are: zero."""
    hs, vs, mcux, mcuy, grids = geometry(p)
    bases = np.concatenate([[0], np.cumsum([h * w for h, w in grids])])
    coef = np.zeros((int(bases[-1]), 64), dtype=np.int16)
    total = mcux * mcuy
    interval = p.interval if p.interval else total
    dc = [_table(p.huff[(0, s[0])]) for s in p.scan]
    ac = [_table(p.huff[(1, s[1])]) for s in p.scan]
    status = 0
    for s, (begin, end) in enumerate(p.segments):
        first = s * interval
        if first >= total:
            break
        # unstuff up to the first marker; behind the real bits come made-up zeros
        raw = data[begin:end]
        cut = len(raw)
        k = raw.find(b"\xff")
        while k != -1:
            if k + 1 < len(raw) and raw[k + 1] == 0:
                k = raw.find(b"\xff", k + 2)
            else:
                cut = k
                break
        real = raw[:cut].replace(b"\xff\x00", b"\xff")
        nreal = 8 * len(real)
        bits = int.from_bytes(real + b"\0" * 8, "big")
        nbits = nreal + 64
        at = 0                                                   # bits consumed

        def symbol(table):
            nonlocal at
            if at + 16 > nbits:
                return ST_TRUNCATED, 0
            hit = table[(bits >> (nbits - at - 16)) & 0xFFFF]
            if hit is None:
                return ST_BADCODE, 0
            at += hit[0]
            return (ST_TRUNCATED if at > nreal else 0), hit[1]

        def take(n):
            nonlocal at
            v = (bits >> (nbits - at - n)) & ((1 << n) - 1) if n else 0
            at += n
            return (ST_TRUNCATED if at > nreal else 0), v

        st = 0
        pred = [0] * len(p.comps)
        for mcu in range(first, min(first + interval, total)):
            my, mx = divmod(mcu, mcux)
            for c in range(len(p.comps)):
                ch, cv = (hs, vs) if c == 0 else (1, 1)
                for b in range(ch * cv):
                    block = coef[bases[c] + (my * cv + b // ch) * grids[c][1] + mx * ch + b % ch]
                    st, sym = symbol(dc[c])
                    if st:
                        break
                    st, v = take(sym & 15)
                    if st:
                        break
                    pred[c] += _extend(v, sym & 15)
                    block[0] = np.int16(((pred[c] + 32768) & 0xFFFF) - 32768)
                    k = 1
                    while k <= 63:
                        st, sym = symbol(ac[c])
                        if st:
                            break
                        run, size = sym >> 4, sym & 15
                        if size == 0:
                            if run != 15:
                                break
                            k += 16
                            if k > 64:
                                st = ST_RUN
                                break
                        else:
                            k += run
                            if k > 63:
                                st = ST_RUN
                                break
                            st, v = take(size)
                            if st:
                                break
                            block[NATURAL[k]] = _extend(v, size)
                            k += 1
                    if st:
                        break
                if st:
                    break
            if st:
                break
        status |= st
    return coef, status


def _idct_1d(x, shift):
    """jidctint's 1-D pass on the leading axis of an int64 array (8, ...)."""
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * -15137
    tmp3 = z1 + z2 * 6270
    tmp0 = (x[0] + x[4]) << 13
    tmp1 = (x[0] - x[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    r = 1 << (shift - 1)
    return np.stack([(tmp10 + tmp3 + r) >> shift, (tmp11 + tmp2 + r) >> shift, (tmp12 + tmp1 + r) >> shift, (tmp13 + tmp0 + r) >> shift,
                     (tmp13 - tmp0 + r) >> shift, (tmp12 - tmp1 + r) >> shift, (tmp11 - tmp2 + r) >> shift, (tmp10 - tmp3 + r) >> shift])


def planes(coef, p):
    """Dequantise + IDCT + range limit: one uint8 plane per component, padded to whole blocks."""
    _, _, _, _, grids = geometry(p)
    out, base = [], 0
    for c, (gh, gw) in enumerate(grids):
        blocks = coef[base:base + gh * gw].astype(np.int64) * p.qt[p.comps[c][3]][None, :]
        base += gh * gw
        x = blocks.reshape(-1, 8, 8)                             # [block][row][col]
        w = _idct_1d(x.transpose(1, 0, 2), 11)                   # pass 1: along the rows' index (columns), -> [row][block][col]
        y = _idct_1d(w.transpose(2, 1, 0), 18)                   # pass 2: along the columns' index (rows), -> [col][block][row]
        i = (y.transpose(1, 2, 0) + 128) & 1023                  # [block][row][col]
        s = np.where(i < 256, i, np.where(i < 640, 255, 0)).astype(np.uint8)
        out.append(s.reshape(gh, gw, 8, 8).transpose(0, 2, 1, 3).reshape(gh * 8, gw * 8))
    return out


def _upsample_h(t, bias_even, bias_odd, shift, centre):
    """The horizontal triangle filter on rows t (int64 (rows, cw)): even outputs (3 c + left + bias_even) >> shift, odd outputs
    (3 c + right + bias_odd) >> shift; the two end samples are (centre c + bias) >> shift."""
    rows, cw = t.shape
    out = np.empty((rows, 2 * cw), dtype=np.int64)
    out[:, 2::2] = (3 * t[:, 1:] + t[:, :-1] + bias_even) >> shift
    out[:, 1:-1:2] = (3 * t[:, :-1] + t[:, 1:] + bias_odd) >> shift
    out[:, 0] = (centre * t[:, 0] + bias_even) >> shift
    out[:, -1] = (centre * t[:, -1] + bias_odd) >> shift
    return out


def upsample(plane, p, hs, vs):
    """A chroma plane -> (H, W) at full resolution.  Edges replicate at the component's downsampled size; libjpeg takes the fancy
    filter only for a downsampled width above 2."""
    cw, ch = -(-p.width // hs), -(-p.height // vs)
    t = plane[:ch, :cw].astype(np.int64)
    if hs == 1:
        return t[:p.height, :p.width]
    if cw <= 2:
        return np.repeat(np.repeat(t, vs, axis=0), 2, axis=1)[:p.height, :p.width]
    if vs == 1:
        out = _upsample_h(t, 1, 2, 2, 4)
        out[:, 0], out[:, -1] = t[:, 0], t[:, -1]
        return out[:p.height, :p.width]
    above = np.concatenate([t[:1], t[:-1]])
    below = np.concatenate([t[1:], t[-1:]])
    rows = np.empty((2 * ch, cw), dtype=np.int64)
    rows[0::2] = 3 * t + above
    rows[1::2] = 3 * t + below
    return _upsample_h(rows, 8, 7, 4, 4)[:p.height, :p.width]


def decode(data):
    """bytes of a baseline JPEG -> (image as PIL gives it: uint8 (H, W) or (H, W, 3); status)."""
    p = parse(data)
    coef, status = entropy(data, p)
    return pixels(coef, p), status


def pixels(coef, p):
    pl = planes(coef, p)
    y = pl[0][:p.height, :p.width].astype(np.int64)
    if len(pl) == 1:
        return y.astype(np.uint8)
    hs, vs = p.comps[0][1], p.comps[0][2]
    cb = upsample(pl[1], p, hs, vs) - 128
    cr = upsample(pl[2], p, hs, vs) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


# ---- the test images -------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (8, 9), (16, 16), (17, 23), (33, 50), (40, 41), (48, 64)]


def make_array(height, width, mode, seed):
    """A smooth pattern plus noise: every AC position gets coefficients, and high qualities get long codes."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    chans = 1 if mode == "L" else 3
    base = np.stack([127 + 90 * np.sin(0.21 * xx + 0.5 * k) * np.cos(0.13 * yy - 0.3 * k) for k in range(chans)], axis=-1)
    img = np.clip(base + rng.normal(0, 28, base.shape), 0, 255).astype(np.uint8)
    return img[:, :, 0] if mode == "L" else img


def make_jpeg(height, width, subsampling=0, quality=75, optimize=False, restart=0, seed=0, mode=None, **extra):
    """PIL-encoded bytes; subsampling 0 / 1 / 2 = 4:4:4 / 4:2:2 / 4:2:0, 'L' = grayscale."""
    import io
    from PIL import Image
    mode = mode or ("L" if subsampling == "L" else "RGB")
    kw = dict(quality=quality, optimize=optimize, **extra)
    if mode == "RGB":
        kw["subsampling"] = subsampling
    if restart:
        kw["restart_marker_blocks"] = restart
    buf = io.BytesIO()
    Image.fromarray(make_array(height, width, mode, seed)).save(buf, "JPEG", **kw)
    return buf.getvalue()


def grid():
    """The 448 files of the issue's grid as (key, bytes): 7 sizes x (4:4:4, 4:2:2, 4:2:0, L) x quality (30, 75, 95, 100) x optimize x
    restart_marker_blocks (0, 2)."""
    out, seed = [], 0
    for (h, w) in SIZES:
        for sub in (0, 1, 2, "L"):
            for q in (30, 75, 95, 100):
                for opt in (False, True):
                    for rst in (0, 2):
                        seed += 1
                        out.append(((h, w, sub, q, opt, rst), make_jpeg(h, w, sub, q, opt, rst, seed)))
    return out


def pil_decode(data):
    import io
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im, dtype=np.uint8)
