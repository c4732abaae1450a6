"""numpy restatement of the device half of the JPEG decoder (hippomm_amd/csrc/jpeg.hip): coefficient slot -> RGB u8 by
libjpeg-turbo's arithmetic under Pillow's defaults -- jidctint.c (islow), jdsample.c (fancy h2v1 / h2v2 upsampling, plain
replication when the chroma is 2 samples wide or less), jdcolor.c (fixed-point YCbCr -> RGB).  The slot layout is restated from
hippomm_amd/csrc/jpeg_layout.h.  Slow and plain: it pins the arithmetic against Pillow on a machine without a GPU."""
import numpy as np

QT_BYTES = 512


def _cdiv(a, b):
    return -(-a // b)


def layout(geometry, window):
    """jpeg_layout: per component (cw, ch, bx0, by0, nbx, nby, first block), plus blocks per frame and the slot size."""
    W, H, ncomp, hmax, vmax = (int(v) for v in geometry[:5])
    if ncomp == 1:
        hmax = vmax = 1
    x0, y0, w, h = window
    mcux, mcuy = _cdiv(W, 8 * hmax), _cdiv(H, 8 * vmax)
    comps, blocks = [], 0
    fancy = False
    for c in range(ncomp):
        hc, vc = (hmax, vmax) if c == 0 else (1, 1)
        cw, ch = _cdiv(W * hc, hmax), _cdiv(H * vc, vmax)
        sx0, sx1, sy0, sy1 = x0, x0 + w, y0, y0 + h
        if c > 0:
            fancy = cw > 2
            halo = 1 if fancy else 0
            if hmax == 2:
                sx0, sx1 = (x0 >> 1) - halo, ((x0 + w - 1) >> 1) + 1 + halo
            if vmax == 2:
                sy0, sy1 = (y0 >> 1) - halo, ((y0 + h - 1) >> 1) + 1 + halo
            sx0, sy0, sx1, sy1 = max(sx0, 0), max(sy0, 0), min(sx1, cw), min(sy1, ch)
        bx0, by0 = sx0 // 8, sy0 // 8
        nbx, nby = _cdiv(sx1, 8) - bx0, _cdiv(sy1, 8) - by0
        comps.append(dict(cw=cw, ch=ch, bx0=bx0, by0=by0, nbx=nbx, nby=nby, first=blocks))
        blocks += nbx * nby
    slot = _cdiv(QT_BYTES + blocks * 128, 256) * 256
    return dict(ncomp=ncomp, rx=hmax, ry=vmax, fancy=fancy, comps=comps, blocks=blocks, slot_bytes=slot)


def _islow_1d(d):
    """jidctint.c's butterfly on the last axis (int64) -> the 8 outputs before descaling."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., k] for k in range(8))
    z1 = (d2 + d6) * 4433
    tmp2 = z1 + d6 * -15137
    tmp3 = z1 + d2 * 6270
    tmp0, tmp1 = (d0 + d4) * 8192, (d0 - d4) * 8192
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = d7, d5, d3, d1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    return np.stack([tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3], axis=-1)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def idct_islow(coefs, q):
    """coefs (..., 64) int16 natural order, q (64,) -> (..., 8, 8) u8 samples."""
    d = coefs.astype(np.int64).reshape(-1, 8, 8) * q.astype(np.int64).reshape(8, 8)
    ws = _descale(_islow_1d(d.transpose(0, 2, 1)), 11).transpose(0, 2, 1)        # pass 1 on columns
    v = _descale(_islow_1d(ws), 18)                                                # pass 2 on rows
    # range limit as libjpeg-turbo's SIMD IDCT applies it (saturation); jidctint.c's table (v & 1023) agrees for |v| < 384
    return (np.clip(v, -128, 127) + 128).astype(np.uint8).reshape(coefs.shape[:-1] + (8, 8))


def reconstruct(slot, geometry, window):
    """One coefficient slot (bytes or u8 array) -> the window (h, w, 3) u8."""
    L = layout(geometry, window)
    raw = np.frombuffer(bytes(slot), dtype=np.uint8)
    qt = raw[:384].view(np.uint16).reshape(3, 64)
    coefs = raw[QT_BYTES:QT_BYTES + L["blocks"] * 128].view(np.int16).reshape(-1, 64)
    x0, y0, w, h = window
    planes = []
    for c, comp in enumerate(L["comps"]):
        blk = idct_islow(coefs[comp["first"]:comp["first"] + comp["nbx"] * comp["nby"]], qt[c])
        blk = blk.reshape(comp["nby"], comp["nbx"], 8, 8).transpose(0, 2, 1, 3).reshape(comp["nby"] * 8, comp["nbx"] * 8)
        planes.append(blk.astype(np.int64))
    X = np.arange(x0, x0 + w)[None, :]
    Y = np.arange(y0, y0 + h)[:, None]

    def at(c, sx, sy):
        comp = L["comps"][c]
        return planes[c][sy - comp["by0"] * 8, sx - comp["bx0"] * 8]

    y = at(0, X, Y)
    if L["ncomp"] == 1:
        return np.repeat(y.astype(np.uint8)[:, :, None], 3, axis=2)

    def chroma(c):
        comp = L["comps"][c]
        if L["rx"] == 1:
            return at(c, X, Y)
        i, odd = X >> 1, X & 1
        j = (Y >> 1) if L["ry"] == 2 else Y
        if not L["fancy"]:
            return at(c, i, j)
        other = np.where(odd == 1, np.minimum(i + 1, comp["cw"] - 1), np.maximum(i - 1, 0))
        if L["ry"] == 1:
            return (3 * at(c, i, j) + at(c, other, j) + 1 + odd) >> 2
        jn = np.where((Y & 1) == 1, np.minimum(j + 1, comp["ch"] - 1), np.maximum(j - 1, 0))
        near = 3 * at(c, i, j) + at(c, i, jn)
        far = 3 * at(c, other, j) + at(c, other, jn)
        return (3 * near + far + 8 - odd) >> 4

    cb, cr = chroma(1) - 128, chroma(2) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)
