"""A numpy restatement, serial and slow, of the JPEG decoder include/rtv_hip_jpeg_decode.h describes, written from the standards
and from libjpeg's documented arithmetic, independent of the native code (the tests compare the two):

  * ITU-T T.81: B.2 marker segments, C.2 code generation, F.2.2 Huffman decoding of DC differences and AC coefficients (EXTEND,
    run / size symbols, ZRL, EOB), F.1.2.3 byte stuffing, E.2.4 restart intervals, A.3.6 zigzag order;
  * libjpeg (jidctint.c, jdsample.c, jdcolor.c), the decoder behind PIL: the "islow" integer inverse DCT (CONST_BITS 13,
    PASS1_BITS 2) on the dequantised coefficients with its 10-bit range-limit table, "fancy" triangle-filter upsampling (h2v1:
    (3 a + b + 1 or 2) >> 2; h2v2: the same weights in both directions, (. + 8 or 7) >> 4; the edge sample replicated, at the TRUE
    size of the subsampled plane), and the 16-bit fixed-point Y Cb Cr -> RGB tables.

Coefficients: one int16 array [block_rows, block_cols, 64] per component, natural order, over the padded block grid.

The second half of the file holds what the CPU and the GPU tests share: the valid and the damaged test files, and the runner of
the host check program (csrc/jpeg_decode_hostcheck.cpp)."""
import io
import os
import subprocess

import numpy as np

import jpeg_oracle as jo

ZIGZAG = jo.ZIGZAG


class Refused(ValueError):
    """A file outside the accepted subset (the parser's answer)."""


class ScanError(ValueError):
    """A damaged scan (the serial decoder's answer)."""


# ------------------------------------------------------------------------------------------------------------------- the header
def parse(data):
    """-> dict(H, W, ncomp, hs, vs, ri, quant=[ncomp][64] natural, dc=[ncomp] (BITS, HUFFVAL), ac=..., scan=bytes)."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise Refused("no SOI")
    at, qt, huff, ri, sof, adobe = 2, {}, {}, 0, None, None
    while True:
        if at + 4 > len(data):
            raise Refused("truncated header")
        if data[at] != 0xFF:
            raise Refused("malformed header")
        m = data[at + 1]
        if m == 0xFF:
            at += 1
            continue
        if m in (0xD8, 0x01) or 0xD0 <= m <= 0xD7:
            at += 2
            continue
        n = int.from_bytes(data[at + 2:at + 4], "big")
        p = data[at + 4:at + 2 + n]
        if n < 2 or at + 2 + n > len(data):
            raise Refused("truncated header")
        at += 2 + n
        if m == 0xC0:
            if p[0] != 8:
                raise Refused("precision")
            sof = dict(H=int.from_bytes(p[1:3], "big"), W=int.from_bytes(p[3:5], "big"),
                       comps=[(p[6 + 3 * c], p[7 + 3 * c] >> 4, p[7 + 3 * c] & 15, p[8 + 3 * c]) for c in range(p[5])])
        elif 0xC1 <= m <= 0xCF and m != 0xC4:
            raise Refused("not baseline (SOF%d)" % (m - 0xC0))
        elif m == 0xC4:
            o = 0
            while o < len(p):
                bits = list(p[o + 1:o + 17])
                huff[(p[o] >> 4, p[o] & 15)] = (bits, list(p[o + 17:o + 17 + sum(bits)]))
                o += 17 + sum(bits)
        elif m == 0xDB:
            o = 0
            while o < len(p):
                if p[o] >> 4:
                    raise Refused("16-bit quantisation table")
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = list(p[o + 1:o + 65])
                qt[p[o] & 15] = t
                o += 65
        elif m == 0xDD:
            ri = int.from_bytes(p[:2], "big")
        elif m == 0xEE and p[:5] == b"Adobe":
            adobe = p[11]
        elif m == 0xDA:
            if sof is None or p[0] != len(sof["comps"]) or len(sof["comps"]) not in (1, 3):
                raise Refused("components")
            if (p[1 + 2 * p[0]], p[2 + 2 * p[0]], p[3 + 2 * p[0]]) != (0, 63, 0):
                raise Refused("not one full scan")
            sel = [(p[2 + 2 * c] >> 4, p[2 + 2 * c] & 15) for c in range(p[0])]
            break
    comps = sof["comps"]
    if len(comps) == 3:
        hs, vs = comps[0][1], comps[0][2]
        if (hs, vs) not in ((1, 1), (2, 1), (2, 2)) or any(c[1:3] != (1, 1) for c in comps[1:]):
            raise Refused("sampling")
        if adobe == 0:
            raise Refused("Adobe transform 0")
    else:
        hs = vs = 1
    try:
        out = dict(H=sof["H"], W=sof["W"], ncomp=len(comps), hs=hs, vs=vs, ri=ri, quant=[qt[c[3]] for c in comps],
                   dc=[huff[(0, s[0])] for s in sel], ac=[huff[(1, s[1])] for s in sel])
    except KeyError:
        raise Refused("missing table")
    # the scan: up to the first marker that is no restart marker
    e = at
    while True:
        e = data.find(b"\xff", e)
        if e < 0 or e + 1 >= len(data):
            e = len(data)
            break
        if data[e + 1] in (0x00, 0xFF) or 0xD0 <= data[e + 1] <= 0xD7:
            e += 1 if data[e + 1] == 0xFF else 2
            continue
        break
    out["scan"] = data[at:e]
    out["mcu_cols"], out["mcu_rows"] = -(-out["W"] // (8 * hs)), -(-out["H"] // (8 * vs))
    return out


# --------------------------------------------------------------------------------------------------------------- entropy decode
def _lut(bits, vals):
    """16-bit window -> (length << 8) | symbol, 0 = no code (T.81 C.2; a code is never all ones, so 0 is free: length >= 1)."""
    lut = np.zeros(65536, np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            lut[code << (16 - length):(code + 1) << (16 - length)] = (length << 8) | vals[k]
            code, k = code + 1, k + 1
        code <<= 1
    return lut


def _segments(scan):
    """The scan cut at its restart markers -> [unstuffed bytes]."""
    out, at = [], 0
    while True:
        e = at
        while True:
            e = scan.find(b"\xff", e)
            if e < 0 or e + 1 >= len(scan):
                e = len(scan)
                break
            if scan[e + 1] == 0x00:
                e += 2
                continue
            break
        out.append(scan[at:e].replace(b"\xff\x00", b"\xff"))
        if e >= len(scan):
            return out
        if not 0xD0 <= scan[e + 1] <= 0xD7:
            return out                                                  # fill bytes or a stray marker: the scan ends here
        at = e + 2


def entropy_decode(info):
    """The serial decoder -> [int16 [block_rows, block_cols, 64]] per component.  Raises ScanError on a damaged scan: a bit pattern
    that is no code, a zigzag index past 63, a segment that ends inside an MCU or holds more than its MCUs, segments missing or
    too many."""
    hs, vs, ncomp, ri = info["hs"], info["vs"], info["ncomp"], info["ri"]
    cols, rows = info["mcu_cols"], info["mcu_rows"]
    coef = [np.zeros((rows * (vs if c == 0 else 1), cols * (hs if c == 0 else 1), 64), np.int16) for c in range(ncomp)]
    dc_lut = [_lut(*t) for t in info["dc"]]
    ac_lut = [_lut(*t) for t in info["ac"]]
    slots = [(0, sy, sx) for sy in range(vs) for sx in range(hs)] + [(c, 0, 0) for c in range(1, ncomp)]
    total = cols * rows
    per = ri if ri else total
    segs = _segments(info["scan"])
    if len(segs) != -(-total // per):
        raise ScanError("%d segments for %d restart intervals" % (len(segs), -(-total // per)))
    mcu = 0
    for seg in segs:
        bits = np.unpackbits(np.frombuffer(seg, np.uint8))
        nbits = len(bits)
        padded = np.concatenate([bits, np.zeros(16, np.uint8)]).astype(np.int64)
        win = np.zeros(nbits + 1, np.int64)
        for k in range(16):
            win += padded[k:k + nbits + 1] << (15 - k)
        pos, pred = 0, [0] * ncomp

        def symbol(lut):
            nonlocal pos
            e = int(lut[win[pos]]) if pos <= nbits else 0
            if e == 0 or pos + (e >> 8) > nbits:
                raise ScanError("no code / out of bits at bit %d of %d" % (pos, nbits))
            pos += e >> 8
            return e & 255

        def value(s):
            nonlocal pos
            if s == 0:
                return 0
            if s > 15 or pos + s > nbits:
                raise ScanError("out of bits")
            v = int(win[pos]) >> (16 - s)
            pos += s
            return v if v >= 1 << (s - 1) else v - (1 << s) + 1

        for m in range(mcu, min(mcu + per, total)):
            my, mx = divmod(m, cols)
            for c, sy, sx in slots:
                blk = coef[c][my * (vs if c == 0 else 1) + sy, mx * (hs if c == 0 else 1) + sx]
                pred[c] += value(symbol(dc_lut[c]))
                blk[0] = pred[c]
                k = 1
                while k < 64:
                    rs = symbol(ac_lut[c])
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        k += 16
                        continue
                    k += r
                    if k > 63:
                        raise ScanError("zigzag index past 63")
                    blk[ZIGZAG[k]] = value(s)
                    k += 1
        if nbits - pos >= 8:
            raise ScanError("a segment holds more than its MCUs")
        mcu = min(mcu + per, total)
    return coef


# ------------------------------------------------------------------------------------------------------------------ pixel stage
def _idct_pass(x, shift):
    """jidctint.c's 8-point pass along the last axis of int64 [..., 8]."""
    z2, z3 = x[..., 2], x[..., 6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * -15137
    tmp3 = z1 + z2 * 6270
    tmp0 = (x[..., 0] + x[..., 4]) << 13
    tmp1 = (x[..., 0] - x[..., 4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[..., 7], x[..., 5], x[..., 3], x[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    rnd = 1 << (shift - 1)
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([(o + rnd) >> shift for o in out], -1)


def idct_islow(coef, quant):
    """int16 [R, C, 64] natural order, steps [64] -> samples uint8 [R * 8, C * 8]."""
    R, C = coef.shape[:2]
    x = (coef.astype(np.int64) * quant.astype(np.int64)).reshape(R, C, 8, 8)
    ws = _idct_pass(x.swapaxes(-1, -2), 11).swapaxes(-1, -2)             # columns
    y = _idct_pass(ws, 18) & 1023                                        # rows, then range_limit[. & RANGE_MASK]
    y = np.where(y < 512, np.minimum(y + 128, 255), np.maximum(y - 896, 0))
    return y.transpose(0, 2, 1, 3).reshape(R * 8, C * 8).astype(np.uint8)


def upsample_fancy(plane, hs, vs):
    """A subsampled plane at its true size [ch, cw] -> [ch * vs, cw * hs] (jdsample.c h2v1 / h2v2 fancy upsampling)."""
    p = np.pad(plane.astype(np.int64), 1, mode="edge")
    if (hs, vs) == (1, 1):
        return plane.astype(np.int64)
    if (hs, vs) == (2, 1):
        c, left, right = p[1:-1, 1:-1], p[1:-1, :-2], p[1:-1, 2:]
        out = np.empty((plane.shape[0], plane.shape[1] * 2), np.int64)
        out[:, 0::2] = (3 * c + left + 1) >> 2
        out[:, 1::2] = (3 * c + right + 2) >> 2
        return out
    out = np.empty((plane.shape[0] * 2, plane.shape[1] * 2), np.int64)
    for v, near in ((0, p[:-2]), (1, p[2:])):                             # output row 2 r + v: the row above / below is the further one
        colsum = 3 * p[1:-1] + near                                      # [ch, cw + 2]
        c, left, right = colsum[:, 1:-1], colsum[:, :-2], colsum[:, 2:]
        out[v::2, 0::2] = (3 * c + left + 8) >> 4
        out[v::2, 1::2] = (3 * c + right + 7) >> 4
    return out


def pixels(info, coef):
    """Coefficients -> rgb8 [H, W, 3]."""
    H, W, hs, vs = info["H"], info["W"], info["hs"], info["vs"]
    y = idct_islow(coef[0], info["quant"][0])[:H, :W].astype(np.int64)
    if info["ncomp"] == 1:
        return np.stack([y, y, y], -1).astype(np.uint8)
    ch, cw = -(-H // vs), -(-W // hs)
    cb, cr = (upsample_fancy(idct_islow(coef[c], info["quant"][c])[:ch, :cw], hs, vs)[:H, :W] - 128 for c in (1, 2))
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data):
    info = parse(data)
    return pixels(info, entropy_decode(info))


def flat(coef):
    """The layout of rtv_jpeg_decode_coefficients: component after component."""
    return np.concatenate([c.reshape(-1) for c in coef])


def from_encoder_layout(co, H, W):
    """jpeg_oracle.coefficients' [mcu_rows, mcus, 6, 64] zigzag -> this module's per-component natural-order planes (4:2:0)."""
    rows, mcus = co.shape[:2]
    nat = np.zeros_like(co)
    nat[..., ZIGZAG] = co
    y = nat[:, :, :4].reshape(rows, mcus, 2, 2, 64).transpose(0, 2, 1, 3, 4).reshape(rows * 2, mcus * 2, 64)
    return [y, nat[:, :, 4], nat[:, :, 5]]


# ---------------------------------------------------------------------------------------------------- test files, shared by tests
SIZES = [(8, 8), (16, 16), (17, 23), (24, 40), (152, 24)]
MODES = {"444": dict(subsampling=0), "422": dict(subsampling=1), "420": dict(subsampling=2), "grey": None}


def pil_file(img, q=90, mode="420", **kw):
    from PIL import Image
    b = io.BytesIO()
    if mode == "grey":
        Image.fromarray(img[..., 1]).save(b, format="JPEG", quality=q, **kw)
    else:
        Image.fromarray(img).save(b, format="JPEG", quality=q, **dict(MODES[mode], **kw))
    return b.getvalue()


def pil_pixels(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(bytes(data))).convert("RGB"))


def valid_files():
    """{name: file}: every sampling mode over SIZES, optimised tables, restart markers per MCU row and every 3 MCUs, the encoder
    oracle's own stream (one restart interval per MCU row), and one 160 x 240 noise image at q 95 whose restart-free scan spans
    hundreds of default-length subsequences."""
    out = {}
    for H, W in SIZES:
        for mode in MODES:
            for kind, q in (("smooth", 90), ("noise", 50)):
                out[f"{mode}_{H}x{W}_{kind}_q{q}"] = pil_file(jo.image(H, W, kind), q, mode)
        img = jo.image(H, W, "smooth", seed=1)
        out[f"420_{H}x{W}_opt"] = pil_file(img, 90, "420", optimize=True)
        out[f"422_{H}x{W}_rst_rows"] = pil_file(img, 100, "422", restart_marker_rows=1)
        out[f"444_{H}x{W}_rst3_opt"] = pil_file(img, 90, "444", restart_marker_blocks=3, optimize=True)
        out[f"420_{H}x{W}_rst3"] = pil_file(img, 90, "420", restart_marker_blocks=3)
        if H % 8 == 0 and W % 8 == 0:
            out[f"own_{H}x{W}"] = jo.encode(img, 90)
    out["420_160x240_noise_q95"] = pil_file(jo.image(160, 240, "noise"), 95, "420")
    return out


def _scan_start(data):
    at = 2
    while True:
        m, n = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        at += 2 + n
        if m == 0xDA:
            return at


def damaged_files():
    """{name: file}, fixed and seeded; each damaged in one of four ways: cut inside the scan, single bits flipped in the scan, a
    marker planted mid-scan, a Huffman table with a code removed."""
    rng = np.random.default_rng(20240611)
    base = {"420": pil_file(jo.image(48, 64, "smooth"), 90, "420"),
            "444rst": pil_file(jo.image(24, 40, "noise"), 75, "444", restart_marker_blocks=3),
            "own": jo.encode(jo.image(48, 64, "smooth", seed=2), 90),
            "grey_opt": pil_file(jo.image(40, 40, "noise"), 90, "grey", optimize=True)}
    out = {}
    for name, data in base.items():
        s, n = _scan_start(data), len(data)
        for frac in (0.1, 0.5, 0.9):                                     # cut: the file ends inside the scan (no EOI)
            out[f"{name}_cut{int(frac * 100)}"] = data[:s + int((n - 2 - s) * frac)]
        for i in range(4):                                               # one bit flipped
            at = int(rng.integers(s, n - 2))
            b = bytearray(data)
            b[at] ^= 1 << int(rng.integers(0, 8))
            out[f"{name}_flip{i}"] = bytes(b)
        for i, marker in enumerate((0xD3, 0xD9, 0xE1, 0xD0)):            # a marker planted over two bytes of the scan
            at = int(rng.integers(s + 1, n - 4))
            b = bytearray(data)
            b[at:at + 2] = bytes([0xFF, marker])
            out[f"{name}_marker{i}"] = bytes(b)
        # a Huffman table that loses its last code: BITS of the longest length goes down by one, the last symbol goes
        at = 2
        while True:
            m, ln = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
            if m == 0xC4:
                p = bytearray(data[at + 4:at + 2 + ln])
                bits = p[1:17]
                count = sum(bits)
                if len(p) == 17 + count:                                 # one table in this segment
                    last = max(i for i in range(16) if bits[i])
                    p[1 + last] -= 1
                    del p[17 + count - 1]
                    out[f"{name}_huff_{p[0]:02x}"] = data[:at + 2] + (ln - 1).to_bytes(2, "big") + bytes(p) + data[at + 2 + ln:]
            if m == 0xDA:
                break
            at += 2 + ln
    return out


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realtime_video_amd", "csrc")


def build_hostcheck(sanitize):
    """make hostcheck [SANITIZE=1] -> the program's path, or None when no host compiler builds it."""
    r = subprocess.run(["make", "-C", CSRC, "hostcheck"] + (["SANITIZE=1"] if sanitize else []), capture_output=True, text=True)
    path = os.path.join(CSRC, "build", "jpeg_decode_hostcheck_san" if sanitize else "jpeg_decode_hostcheck")
    return path if r.returncode == 0 and os.path.exists(path) else None


def run_hostcheck(program, files, subseq_bits, workdir):
    """files {name: bytes} through ONE child process -> (returncode, stderr, {name: ("refused", reason) | (status, rounds, int16
    coefficients)})."""
    os.makedirs(workdir, exist_ok=True)
    paths = []
    for name, data in files.items():
        paths.append(os.path.join(workdir, name + ".jpg"))
        with open(paths[-1], "wb") as f:
            f.write(data)
    r = subprocess.run([program, str(subseq_bits), workdir] + paths, capture_output=True, text=True)
    out = {}
    for line in r.stdout.splitlines():
        path, what, rest = line.split(" ", 2)
        name = os.path.basename(path)[:-4]
        if what == "refused":
            out[name] = ("refused", rest)
        else:
            w = rest.split()
            out[name] = (int(w[0]), int(w[2]), np.fromfile(os.path.join(workdir, name + ".jpg.coef"), np.int16))
    return r.returncode, r.stderr, out
