"""The colour coding of flows on the device (dfx_flow_colour_device, denseflow_amd/csrc/flow_colour_kernels.hip) against its
NumPy reference (tests/flow_colour_ref.py): the images byte for byte, the n + 1 words of d_max2 bit for bit.  Sizes are the
smallest at which the kernels can go wrong — one pixel, a row shorter than a lane's four pixels, odd widths with a ragged tail,
several workgroups of rows in both passes (4 rows per workgroup of the colour pass, 16 of the measuring pass), and 261 x 5 for
a second 256-pixel workgroup column — in every memory layout that selects another access width: dense, unaligned (single
elements), aligned (16-byte loads of u and v, 4-byte mask and frame loads, 4-byte stores).  The padding of the flows is NaN and
that of the masks 0xFF, so a read of it would show in a maximum or in a colour; the guard bands around d_out and d_max2 must
stay as they were."""
import numpy as np
import pytest

from tests import flow_colour_ref as R
from tests.devmem import DevBuf
from tests.fb_check_ref import smooth_flow

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = [(1, 1), (3, 2), (65, 17), (97, 61), (130, 97), (261, 5)]
MEMS = ["dense", "scalar", "vector"]
GUARD = 64  # elements in front of and behind every output buffer
OUT_FILL, MAX_FILL = 0xA5, F32(-777.25)
UNKNOWN = (17, 99, 201)
ORDERS, LAYOUTS = {"bgr": 0, "rgb": 1}, {"hwc": 0, "chw": 1}
# (order, layout of the images, frame: None / "gray" / "hwc" / "chw", alpha256): every pair of choices occurs
FORMS = [("rgb", "hwc", None, 256), ("bgr", "chw", None, 256), ("bgr", "hwc", "gray", 77), ("rgb", "chw", "gray", 0),
         ("rgb", "hwc", "hwc", 256), ("bgr", "chw", "hwc", 77), ("rgb", "chw", "chw", 128), ("bgr", "hwc", "chw", 201)]

_case_cache = {}


def _case(w, h, n):
    """Flows, masks and frames of one (size, n), computed once and never changed: smooth fields, with n = 3 the middle flow
    three times as large (the batch maximum sits there), the special values planted in the last flow (but the known 1e9,
    which would be every maximum: test_the_seam_subnormals_and_random_bit_patterns has it); a mask over about a fifth of the
    pixels; a gray and a 3-channel frame per flow."""
    key = (w, h, n)
    if key not in _case_cache:
        rng = np.random.default_rng(1000 * w + 10 * h + n)
        flows = smooth_flow(rng, n, h, w, 6.0)
        if n == 3:
            flows[1] *= F32(3)
        R.plant_specials(flows[-1], skip=("1e9",))
        mask = (rng.random((n, h, w)) < 0.2).astype(np.uint8) * rng.integers(1, 256, (n, h, w)).astype(np.uint8)
        gray = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
        colour = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        for a in (flows, mask, gray, colour):
            a.setflags(write=False)
        _case_cache[key] = (flows, mask, gray, colour)
    return _case_cache[key]


def _up4(v):
    return (v + 3) // 4 * 4


def _flow_geom(mem, w, h):
    """(lead floats, row pitch, plane stride, flow stride) as tests/test_fb_check_gpu.py lays flows out."""
    p3, p4 = w + 3, _up4(w) + 4
    return {"dense": (0, w, h * w, 2 * h * w),
            "scalar": (1, p3, h * p3 + 5, 2 * (h * p3 + 5) + 7),  # a base one float in, odd pitches: single elements
            "vector": (0, p4, h * p4 + 8, 2 * (h * p4 + 8) + 12)}[mem]  # everything a multiple of 4 floats


def _byte_geom(mem, kind, w, h):
    """(lead bytes, pitch, plane stride, image stride) of byte images: kind "gray" (also the masks), "hwc" or "chw"."""
    row = 3 * w if kind == "hwc" else w
    planes = 3 if kind == "chw" else 1
    if mem == "dense":
        return 0, row, (h * row if planes == 3 else 0), planes * h * row
    if mem == "scalar":  # a base one byte in and odd strides: every access is a single byte
        pitch = (row + 2) | 1
        plane = h * pitch + 3
        return 1, pitch, (plane if planes == 3 else 0), (planes * plane + 5 if planes == 3 else plane)
    pitch = _up4(row) + 4  # everything a multiple of 4 bytes from an aligned base
    plane = h * pitch + 4
    return 0, pitch, (plane if planes == 3 else 0), (planes * plane + 8 if planes == 3 else plane)


def _pack_flows(flows, geom):
    lead, pitch, plane, stride = geom
    n, _, h, w = flows.shape
    buf = np.full(lead + n * stride + 4, np.nan, F32)  # NaN padding: a read of it would show
    for i in range(n):
        for p in range(2):
            o = lead + i * stride + p * plane
            buf[o:o + h * pitch].reshape(h, pitch)[:, :w] = flows[i, p]
    return buf


def _windows(kind, n, w, h, geom, base=0):
    """Every row of every image (plane) of a padded byte buffer: yields (slice of the buffer, i, y, c or None)."""
    lead, pitch, plane, image = geom
    for i in range(n):
        for c in ((0, 1, 2) if kind == "chw" else (None,)):
            for y in range(h):
                o = base + lead + i * image + (c or 0) * plane + y * pitch
                yield slice(o, o + (3 * w if kind == "hwc" else w)), i, y, c


def _pack_bytes(img, kind, geom, fill):
    """img: (n, h, w) for "gray", (n, h, w, 3) otherwise, into a padded buffer of its memory layout."""
    n, h, w = img.shape[:3]
    lead, pitch, plane, image = geom
    buf = np.full(lead + n * image + 4, fill, np.uint8)
    for s, i, y, c in _windows(kind, n, w, h, geom):
        buf[s] = img[i, y].reshape(-1) if kind != "chw" else img[i, y, :, c]
    return buf


def _unpack_bytes(buf, kind, n, w, h, geom):
    """((n, h, w, 3) image in the memory's channel order, mask of everything outside the windows)."""
    img = np.empty((n, h, w, 3), np.uint8)
    outside = np.ones(buf.shape, bool)
    for s, i, y, c in _windows(kind, n, w, h, geom, GUARD):
        if kind == "chw":
            img[i, y, :, c] = buf[s]
        else:
            img[i, y] = buf[s].reshape(w, 3)
        outside[s] = False
    return img, outside


class _Resident:
    """The inputs of a case on the device in one memory layout, uploaded once."""

    def __init__(self, eng, mem, flows, mask, gray, colour):
        self.eng, self.mem = eng, mem
        self.n, _, self.h, self.w = flows.shape
        w, h = self.w, self.h
        self.fgeom = _flow_geom(mem, w, h)
        self.mgeom = _byte_geom(mem, "gray", w, h)
        self.bufs = {"flow": DevBuf(eng, init=_pack_flows(flows, self.fgeom)),
                     "mask": DevBuf(eng, init=_pack_bytes(mask, "gray", self.mgeom, 0xFF))}  # 0xFF padding: masked if read
        self.frames = {"gray": gray, "hwc": colour, "chw": colour}
        for kind in ("gray", "hwc", "chw"):
            self.bufs[kind] = DevBuf(eng, init=_pack_bytes(self.frames[kind], kind, _byte_geom(mem, kind, w, h), 0x5A))

    def close(self):
        for b in self.bufs.values():
            b.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def run(self, norm, max_rad=0.0, masked=False, order="rgb", layout="hwc", frame=None, alpha256=256, want_max=True,
            unknown=UNKNOWN):
        """(images (n, h, w, 3) in the output's channel order, max2 words or None); checks the guard bands."""
        eng, n, w, h = self.eng, self.n, self.w, self.h
        ogeom = _byte_geom(self.mem, layout, w, h)
        out_host = np.full(2 * GUARD + ogeom[0] + n * ogeom[3] + 4, OUT_FILL, np.uint8)
        max_host = np.full(2 * GUARD + n + 1, MAX_FILL, F32)
        fl, rp, ps, fs = self.fgeom
        ml, mp, _, ms = self.mgeom
        fr = _byte_geom(self.mem, frame, w, h) if frame else (0, 0, 0, 0)
        with DevBuf(eng, init=out_host) as d_out, DevBuf(eng, init=max_host) as d_max:
            eng.flow_colour_device(
                self.bufs["flow"].ptr(4 * fl), rp, ps, fs, n, d_out.ptr(GUARD + ogeom[0]), ogeom[1], ogeom[2], ogeom[3],
                R.NORMS[norm], max_rad, d_max.ptr(4 * GUARD) if want_max else None, ORDERS[order], LAYOUTS[layout], unknown,
                self.bufs["mask"].ptr(ml) if masked else None, mp, ms,
                self.bufs[frame].ptr(fr[0]) if frame else None, (1 if frame == "gray" else 3) if frame else 0,
                LAYOUTS.get(frame, 0), fr[1], fr[2], fr[3], alpha256)
            out_buf, max_buf = d_out.get(np.uint8), d_max.get(F32)
        img, outside = _unpack_bytes(out_buf, layout, n, w, h, ogeom)
        assert np.all(out_buf[outside] == OUT_FILL), "a byte outside the images was written"
        words = max_buf.view(np.uint32)
        fill = np.array([MAX_FILL], F32).view(np.uint32)[0]
        assert np.all(words[:GUARD] == fill) and np.all(words[GUARD + n + 1:] == fill), "the guard bands of d_max2 were written"
        if not want_max:
            assert np.all(words == fill), "d_max2 was written without being asked for"
            return img, None
        return img, max_buf[GUARD:GUARD + n + 1].copy()


def _reference(flows, mask, frames, norm, max_rad, masked, order, frame, alpha256):
    return R.flow_colour(flows, norm, max_rad, mask if masked else None, order, "hwc", UNKNOWN,
                         frames[frame] if frame else None, "hwc", alpha256)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("w,h", SIZES)
def test_the_device_equals_the_reference_in_every_layout(dfx, w, h, n):
    flows, mask, gray, colour = _case(w, h, n)
    frames = {"gray": gray, "hwc": colour, "chw": colour}
    m2_open = R.max2(flows)
    if n == 3 and w * h >= 8:
        assert m2_open[3] == m2_open[1] > max(m2_open[0], m2_open[2])  # the batch maximum sits in the middle flow
    fixed_rad = 4.0  # well inside the flows' range: both branches of the FIXED mode are taken
    refs = {}
    with dfx.FlowEngine(w, h, "farn") as eng:
        for mem in MEMS:
            with _Resident(eng, mem, flows, mask, gray, colour) as dev:
                for norm in ("fixed", "flow", "batch"):
                    rad = fixed_rad if norm == "fixed" else 0.0
                    for masked in (False, True):
                        for order, layout, frame, a256 in FORMS:
                            key = (norm, masked, order, frame, a256)
                            if key not in refs:
                                refs[key] = _reference(flows, mask, frames, norm, rad or None, masked, order, frame, a256)
                            img_ref, m2_ref = refs[key]
                            img, m2 = dev.run(norm, rad, masked, order, layout, frame, a256)
                            bad = img != img_ref
                            assert not bad.any(), (mem, key, layout, int(bad.sum()), img[bad][:6], img_ref[bad][:6])
                            assert _same_bits(m2, m2_ref), (mem, key, m2, m2_ref)
                # FIXED without d_max2: only the colour pass runs, nothing is reported
                img, none = dev.run("fixed", fixed_rad, True, "rgb", "hwc", None, 256, want_max=False)
                assert none is None and np.array_equal(img, refs[("fixed", True, "rgb", None, 256)][0]), mem
    known = R.known(flows, mask)
    print(f"{w}x{h} n={n}: known {known.mean():.3f}, radii {np.sqrt(m2_open)}")


@pytest.mark.parametrize("where", ["first", "last", "tail"])
@pytest.mark.parametrize("w,h", [(97, 61), (261, 5)])
def test_the_maximum_is_found_wherever_it_sits(dfx, w, h, where):
    """The largest vector in the first pixel, in the last pixel of the last row, and in a ragged tail lane (w = 4 k + 1: the
    last lane of a row holds one pixel) of a middle row."""
    n = 2
    rng = np.random.default_rng(w + h)
    flows = smooth_flow(rng, n, h, w, 2.0)
    y, x = {"first": (0, 0), "last": (h - 1, w - 1), "tail": (h // 2, w - 1)}[where]
    assert w % 4 == 1
    flows[1, :, y, x] = (-300.0, 400.0)
    mask = np.zeros((n, h, w), np.uint8)
    gray, colour = np.zeros((n, h, w), np.uint8), np.zeros((n, h, w, 3), np.uint8)
    img_ref, m2_ref = R.flow_colour(flows, "flow", unknown=UNKNOWN)
    assert m2_ref[1] == F32(250000) and m2_ref[2] == m2_ref[1] and m2_ref[0] < 16
    mask_off = mask.copy()
    mask_off[1, y, x] = 1
    img_off, m2_off = R.flow_colour(flows, "flow", mask=mask_off, unknown=UNKNOWN)
    assert m2_off[1] < 16
    with dfx.FlowEngine(w, h, "farn") as eng:
        for mem in MEMS:
            with _Resident(eng, mem, flows, mask, gray, colour) as dev:
                for masked in (False, True):  # an all-zero mask changes nothing
                    img, m2 = dev.run("flow", masked=masked)
                    assert _same_bits(m2, m2_ref) and np.array_equal(img, img_ref), (mem, masked)
            with _Resident(eng, mem, flows, mask_off, gray, colour) as dev:  # the maximum masked: the rest changes colour
                img, m2 = dev.run("flow", masked=True)
                assert _same_bits(m2, m2_off) and np.array_equal(img, img_off), mem


def _special_flows(w, h):
    """Six flows: rows of u = 1 with v = +0 / -0 (the seam of the wheel); subnormal vectors; random bit patterns; all
    unknown; all zero; a smooth flow with every special value of the CPU test, the known 1e9 among them."""
    rng = np.random.default_rng(99)
    fl = np.zeros((6, 2, h, w), F32)
    fl[5] = smooth_flow(rng, 1, h, w, 6.0)[0]
    where = R.plant_specials(fl[5])
    assert len(set(where.values())) == len(R.SPECIALS)
    fl[0, 0] = 1.0
    fl[0, 1, 0::2] = 0.0
    fl[0, 1, 1::2] = -0.0
    tiny = rng.integers(1, 1 << 23, (2, h, w)).astype(np.uint32) | (rng.integers(0, 2, (2, h, w)).astype(np.uint32) << 31)
    fl[1] = tiny.view(F32)
    fl[2] = rng.integers(0, 1 << 32, (2, h, w), dtype=np.uint64).astype(np.uint32).view(F32)
    fl[3] = np.nan
    fl[3, 0, ::2] = np.inf
    return fl


@pytest.mark.parametrize("mem", MEMS)
def test_the_seam_subnormals_and_random_bit_patterns(dfx, mem):
    w, h = 65, 17
    fl = _special_flows(w, h)
    n = fl.shape[0]
    mask = np.zeros((n, h, w), np.uint8)
    gray, colour = np.zeros((n, h, w), np.uint8), np.zeros((n, h, w, 3), np.uint8)
    with dfx.FlowEngine(w, h, "farn") as eng, _Resident(eng, mem, fl, mask, gray, colour) as dev:
        for norm, rad in (("flow", 0.0), ("batch", 0.0), ("fixed", 1e-6), ("fixed", 1.0), ("fixed", 1e9)):
            img_ref, m2_ref = R.flow_colour(fl, norm, rad or None, unknown=UNKNOWN)
            img, m2 = dev.run(norm, rad)
            bad = img != img_ref
            assert not bad.any(), (norm, rad, int(bad.sum()), np.argwhere(bad)[:4], img[bad][:6], img_ref[bad][:6])
            assert _same_bits(m2, m2_ref), (norm, rad, m2, m2_ref)
            if norm == "flow":
                assert np.all(img[0, 0::2] == (255, 0, 0)) and np.all(img[0, 1::2] == (255, 0, 43))  # v = +0 / v = -0
                assert np.all(img[3] == UNKNOWN) and np.all(img[4] == 255)
                assert m2[3:5].view(np.uint32).tolist() == [0, 0]
                assert m2[5] == F32(1e9) * F32(1e9)  # 1e9 is known, and then the maximum; one ulp above it is not
    assert 0.2 < R.known(fl[2:3]).mean() < 0.9  # the random patterns are of both kinds


@pytest.mark.parametrize("mem", MEMS)
def test_a_small_fixed_radius_darkens_most_pixels(dfx, mem):
    w, h, n = 97, 61, 2
    flows, mask, gray, colour = (a[:n] for a in _case(w, h, 3))
    rad = 0.25
    img_ref, m2_ref = R.flow_colour(flows, "fixed", rad, mask, "bgr", "hwc", UNKNOWN)
    k = R.known(flows, mask)
    with np.errstate(all="ignore"):
        far = np.hypot(flows[:, 0], flows[:, 1])[k] > rad
    assert far.mean() > 0.9
    with dfx.FlowEngine(w, h, "farn") as eng, _Resident(eng, mem, flows, mask, gray, colour) as dev:
        for want_max in (True, False):
            for layout in ("hwc", "chw"):
                img, m2 = dev.run("fixed", rad, True, "bgr", layout, want_max=want_max)
                assert np.array_equal(img, img_ref), (want_max, layout)
                assert m2 is None if not want_max else _same_bits(m2, m2_ref)


def _stats_bytes(eng):
    return bytes(eng.stats())


def test_every_refusal_returns_its_status_writes_nothing_and_leaves_the_handle_usable(dfx):
    w, h, n = 65, 17, 3
    flows, mask, gray, colour = _case(w, h, n)
    img_ref, m2_ref = R.flow_colour(flows, "flow", mask=mask, unknown=UNKNOWN, frame=colour, alpha256=77)
    with dfx.FlowEngine(w, h, "tvl1") as eng:
        with DevBuf(eng, init=flows) as d_f, DevBuf(eng, init=mask) as d_m, DevBuf(eng, init=colour) as d_fr, \
                DevBuf(eng, init=np.full(n * h * w * 3, OUT_FILL, np.uint8)) as d_out, \
                DevBuf(eng, init=np.full(n + 1, MAX_FILL, F32)) as d_max:
            good = dict(f=d_f.ptr(), rp=w, ps=h * w, fs=2 * h * w, n=n, out=d_out.ptr(), op=3 * w, opl=0, oi=3 * h * w, norm=1,
                        rad=0.0, max2=d_max.ptr(), order=1, layout=0, unknown=UNKNOWN, mask=d_m.ptr(), mp=w, ms=h * w,
                        frame=d_fr.ptr(), fc=3, fl=0, fp=3 * w, fpl=0, fi=3 * h * w, a=77)

            def call(**kw):
                a = dict(good, **kw)
                eng.flow_colour_device(a["f"], a["rp"], a["ps"], a["fs"], a["n"], a["out"], a["op"], a["opl"], a["oi"], a["norm"],
                                       a["rad"], a["max2"], a["order"], a["layout"], a["unknown"], a["mask"], a["mp"], a["ms"],
                                       a["frame"], a["fc"], a["fl"], a["fp"], a["fpl"], a["fi"], a["a"])

            bytes_before, stats_before = eng.device_bytes(), _stats_bytes(eng)
            refused = [dict(f=None), dict(out=None), dict(n=-1), dict(norm=3), dict(norm=-1), dict(order=2), dict(order=-1),
                       dict(layout=2), dict(layout=-1), dict(fc=2), dict(fc=0), dict(fl=2), dict(rp=w - 1), dict(ps=h * w - 1),
                       dict(fs=2 * h * w - 1), dict(mp=w - 1), dict(ms=h * w - 1), dict(op=3 * w - 1), dict(oi=3 * h * w - 1),
                       dict(layout=1, op=w, opl=h * w - 1), dict(layout=1, op=w, opl=h * w, oi=3 * h * w - 1),
                       dict(layout=1, op=w - 1, opl=h * w), dict(fp=3 * w - 1), dict(fi=3 * h * w - 1),
                       dict(fl=1, fp=w, fpl=h * w - 1), dict(fc=1, fp=w - 1, fi=h * w), dict(a=-1), dict(a=257),
                       dict(max2=None), dict(norm=2, max2=None)]
            refused += [dict(norm=0, rad=r) for r in (0.0, float("nan"), 1e10, float("inf"), -1.0, 1e-7)]
            for kw in refused:
                with pytest.raises(dfx.DfxError) as e:
                    call(**kw)
                assert e.value.status == 1, kw
            assert np.all(d_out.get() == OUT_FILL), "a refused call wrote an image"
            assert np.all(d_max.get(F32) == MAX_FILL), "a refused call wrote d_max2"
            call(n=0)  # DFX_OK, launches nothing
            call(n=0, f=None, out=None, norm=9, max2=None)
            assert np.all(d_out.get() == OUT_FILL) and np.all(d_max.get(F32) == MAX_FILL), "n = 0 wrote"
            call()
            assert np.array_equal(d_out.get().reshape(n, h, w, 3), img_ref), "the handle is not usable after the refusals"
            assert _same_bits(d_max.get(F32), m2_ref)
            call(norm=0, rad=1e-6, max2=None), call(norm=0, rad=1e9), call(frame=None, fc=0, fl=7, a=999)  # accepted
            assert eng.device_bytes() == bytes_before and _stats_bytes(eng) == stats_before
    with dfx.FlowEngine(w, h, "frames") as eng:
        with DevBuf(eng, init=flows) as d_f, DevBuf(eng, n * h * w * 3) as d_out, DevBuf(eng, 4 * (n + 1)) as d_max:
            with pytest.raises(dfx.DfxError) as e:
                eng.flow_colour_device(d_f.ptr(), w, h * w, 2 * h * w, n, d_out.ptr(), 3 * w, 0, 3 * h * w, 1, 0.0, d_max.ptr())
            assert e.value.status == 4


@pytest.mark.parametrize("algo", ["tvl1", "brox"])
def test_numpy_wrapper_on_every_flow_handle(dfx, algo):
    w, h, n = 65, 17, 3
    flows, mask, gray, colour = _case(w, h, n)
    with dfx.FlowEngine(w, h, algo) as eng:
        img, radii, batch = eng.flow_colour(flows, return_max=True)
        img_ref, m2 = R.flow_colour(flows, "flow")
        assert img.shape == (n, h, w, 3) and img.dtype == np.uint8 and np.array_equal(img, img_ref)
        assert _same_bits(radii, np.sqrt(m2[:n])) and _same_bits(batch, np.sqrt(m2[n]))
        got = eng.flow_colour(flows, "batch", mask=mask, order="bgr", layout="chw", unknown=UNKNOWN, frame=gray, alpha=0.3)
        want, _ = R.flow_colour(flows, "batch", None, mask, "bgr", "chw", UNKNOWN, gray, "hwc", int(round(0.3 * 256)))
        assert got.shape == (n, 3, h, w) and np.array_equal(got, want)
        got, radii, batch = eng.flow_colour(flows, "fixed", 3.0, frame=colour.transpose(0, 3, 1, 2), layout="chw", return_max=True)
        want, m2 = R.flow_colour(flows, "fixed", 3.0, None, "rgb", "chw", (0, 0, 0), colour.transpose(0, 3, 1, 2), "chw", 128)
        assert np.array_equal(got, want) and _same_bits(batch, np.sqrt(m2[n]))


def test_the_legend_disc_equals_the_reference_on_the_same_radial_flow(dfx):
    flow, mask = R.key_flow(65)
    want, _ = R.flow_colour(flow, "flow", mask=mask)
    with dfx.FlowEngine(97, 61, "farn") as eng:  # the handle's own size does not matter
        key = eng.flow_colour_key(65)
    assert key.shape == (65, 65, 3) and np.array_equal(key, want[0])
    assert tuple(key[32, 32]) == (255, 255, 255) and tuple(key[0, 0]) == (0, 0, 0) and tuple(key[32, 64]) == (255, 0, 0)
    with dfx.FlowEngine(65, 65, "farn") as eng:
        assert np.array_equal(eng.flow_colour_key(65), want[0])


def test_the_tensor_wrapper_reads_and_writes_a_strided_slice_where_it_lies(dfx):
    import torch

    w, h, n = 65, 17, 3
    flows, mask, gray, colour = _case(w, h, n)
    dev = torch.device("cuda:0")
    big = torch.full((n + 1, 2, h + 3, w + 5), float("nan"), device=dev)
    view = big[1:, :, 1:h + 1, 2:w + 2]
    view.copy_(torch.from_numpy(flows.copy()))
    bigmask = torch.full((n, h + 2, w + 7), 255, dtype=torch.uint8, device=dev)
    mview = bigmask[:, 1:h + 1, 3:w + 3]
    mview.copy_(torch.from_numpy(mask.copy()))
    frame = torch.from_numpy(colour.copy()).to(dev).permute(0, 3, 1, 2)  # (n, 3, h, w) shape over interleaved memory
    with dfx.FlowEngine(w, h, "farn") as eng:
        for norm, rad, layout in (("flow", None, "hwc"), ("batch", None, "chw"), ("fixed", 2.5, "hwc")):
            want, want_r, want_b = eng.flow_colour(flows, norm, rad, mask=mask, order="bgr", layout=layout, unknown=UNKNOWN,
                                                   frame=colour if layout == "hwc" else colour.transpose(0, 3, 1, 2), alpha=0.7,
                                                   return_max=True)
            got, radii, batch = eng.flow_colour_tensor(view, norm, rad, mask=mview, order="bgr", layout=layout, unknown=UNKNOWN,
                                                       frame=frame if layout == "chw" else frame.permute(0, 2, 3, 1), alpha=0.7,
                                                       return_max=True)
            assert got.dtype == torch.uint8 and got.is_contiguous() and np.array_equal(got.cpu().numpy(), want), norm
            assert _same_bits(radii.cpu().numpy(), want_r) and _same_bits(batch.cpu().numpy(), want_b)
        # out=: a slice of a larger tensor, the rest of which stays as it was
        shape = (n, h + 2, w + 3, 3)
        canvas = torch.full(shape, OUT_FILL, dtype=torch.uint8, device=dev)
        out = canvas[:, 1:h + 1, 2:w + 2]
        res = eng.flow_colour_tensor(view, out=out)
        assert res is out
        host = canvas.cpu().numpy()
        assert np.array_equal(host[:, 1:h + 1, 2:w + 2], R.flow_colour(flows, "flow")[0])
        host[:, 1:h + 1, 2:w + 2] = OUT_FILL
        assert np.all(host == OUT_FILL)
        assert eng.flow_colour_tensor(view[:0]).shape == (0, h, w, 3)
