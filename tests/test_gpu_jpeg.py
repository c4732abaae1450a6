"""GPU: hippomm_amd.decode_jpeg (host entropy pass + hmm_jpeg_reconstruct on gfx950) equals Pillow's
``np.asarray(Image.open(p).convert("RGB"))`` bit for bit over the test matrix; window decodes equal crops; mixed batches keep
their order and Pillow's pixels and errors.  Test files are written here with Pillow's encoder."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from test_cpu_jpeg import LARGE, QUALITIES, SIZES, encode, frame, pillow

pytestmark = pytest.mark.gpu


def _decode(sources, **kw):
    from hippomm_amd import decode_jpeg
    stats = {}
    out = decode_jpeg(sources, device="cuda", stats=stats, **kw)
    frames = [o.cpu().numpy() for o in out]
    return frames, stats


def _assert_equal(sources, **kw):
    frames, stats = _decode(sources, **kw)
    assert len(frames) == len(sources)
    for k, (got, src) in enumerate(zip(frames, sources)):
        np.testing.assert_array_equal(got, pillow(src), err_msg=f"frame {k}")
    return stats


def test_self_check_passes_and_route_is_on():
    from hippomm_amd import jpeg
    data = encode(frame(130, 90, seed=1), quality=90, subsampling=2)
    assert jpeg.route_ok(data, torch.device("cuda"))
    assert jpeg._check["ok"] is True


@pytest.mark.parametrize("subsampling", [0, 1, 2])
def test_matrix_equals_pillow(subsampling):
    sources = [encode(frame(*size, seed=size[0] * 31 + size[1]), quality=q, subsampling=subsampling, optimize=opt)
               for size in SIZES for q in QUALITIES for opt in (False, True)]
    stats = _assert_equal(sources)
    assert stats == {"device": len(sources), "host": 0}


@pytest.mark.parametrize("size", LARGE, ids=[f"{w}x{h}" for w, h in LARGE])
def test_large_frames_in_one_batch(size):
    sources = [encode(frame(*size, seed=s), quality=q, subsampling=sub) for s, (q, sub) in
               enumerate(((90, 2), (90, 2), (75, 2), (95, 1), (30, 0), (100, 2)))]
    out, stats = _decode(sources)
    assert stats["device"] == len(sources)
    for got, src in zip(out, sources):
        np.testing.assert_array_equal(got, pillow(src))


def test_restart_markers_grey_and_metadata():
    sources = []
    for kw in (dict(restart_marker_blocks=1), dict(restart_marker_blocks=5), dict(restart_marker_rows=1),
               dict(restart_marker_rows=2)):
        sources += [encode(frame(1280, 720, seed=3), quality=85, subsampling=2, **kw),
                    encode(frame(15, 17, seed=3), quality=85, subsampling=0, **kw)]
    sources += [encode(frame(*s, seed=5, mode="L"), quality=q) for s in ((1, 1), (7, 9), (130, 90), (1280, 720)) for q in (5, 100)]
    exif = Image.Exif()
    exif[0x010F] = "maker"
    sources.append(encode(frame(130, 90, seed=9), quality=90, exif=exif.tobytes(), icc_profile=b"\0" * 300, comment=b"c"))
    stats = _assert_equal(sources)
    assert stats["device"] == len(sources)


def test_window_equals_crop_of_full_decode():
    rng = np.random.default_rng(3)
    for size, sub in (((1280, 720), 2), ((1920, 1080), 1), ((130, 90), 0), ((15, 17), 2)):
        sources = [encode(frame(*size, seed=s), quality=90, subsampling=sub) for s in range(3)]
        full = [pillow(s) for s in sources]
        for _ in range(4):
            x0, y0 = int(rng.integers(0, size[0])), int(rng.integers(0, size[1]))
            w, h = int(rng.integers(1, size[0] - x0 + 1)), int(rng.integers(1, size[1] - y0 + 1))
            got, stats = _decode(sources, window=(x0, y0, w, h))
            assert stats["device"] == len(sources)
            for g, f in zip(got, full):
                np.testing.assert_array_equal(g, f[y0:y0 + h, x0:x0 + w])


def test_mixed_batch_keeps_order_pixels_and_errors(tmp_path):
    im = frame(130, 90, seed=4)
    supported = encode(im, quality=90, subsampling=2)
    progressive = encode(im, quality=90, progressive=True)
    other_size = encode(frame(64, 48, seed=4), quality=75, subsampling=0)
    cmyk = encode(im.convert("CMYK"), quality=90)
    paths = []
    for k, data in enumerate((supported, progressive, other_size, supported, cmyk)):
        p = tmp_path / f"f{k}.jpg"
        p.write_bytes(data)
        paths.append(str(p))
    frames, stats = _decode(paths)
    assert stats == {"device": 3, "host": 2}
    for got, p in zip(frames, paths):
        np.testing.assert_array_equal(got, np.asarray(Image.open(p).convert("RGB")))

    from hippomm_amd import decode_jpeg
    out = decode_jpeg([supported, supported], device="cuda")
    assert isinstance(out, torch.Tensor) and tuple(out.shape) == (2, 90, 130, 3)
    assert isinstance(decode_jpeg(paths, device="cuda"), list)

    missing = str(tmp_path / "missing.jpg")
    garbage = tmp_path / "garbage.jpg"
    garbage.write_bytes(b"not an image at all")
    truncated = tmp_path / "truncated.jpg"
    truncated.write_bytes(supported[:len(supported) // 2])
    for bad in (missing, str(garbage), str(truncated)):
        with pytest.raises(Exception) as want:
            [np.asarray(Image.open(p).convert("RGB")) for p in paths[:2] + [bad] + paths[2:]]
        with pytest.raises(type(want.value)) as got:
            decode_jpeg(paths[:2] + [bad] + paths[2:], device="cuda")
        assert str(got.value) == str(want.value)


def test_bytes_and_paths_agree(tmp_path):
    data = encode(frame(1280, 720, seed=8), quality=90, subsampling=2)
    p = tmp_path / "a.jpg"
    p.write_bytes(data)
    from hippomm_amd import decode_jpeg
    a = decode_jpeg([data], device="cuda")
    b = decode_jpeg([str(p)], device="cuda")
    assert torch.equal(a, b)
    np.testing.assert_array_equal(a[0].cpu().numpy(), np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))
