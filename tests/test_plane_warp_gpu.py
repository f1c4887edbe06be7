"""The backward warp of float, half and label planes on the device (dfx_warp_planes_device,
denseflow_amd/csrc/plane_warp_kernels.hip) against its NumPy restatement (tests/plane_warp_ref.py): bit for bit, except that of
a bilinear sample that is NaN only the NaN-ness is compared.  Every output buffer is compared WHOLE with the buffer the
reference predicts — the fill in the padding, in the guard bands and, with keep, in the pixels that are not valid — so a
store outside the windows shows like a wrong value.  Device memory is torch's: the library allocates nothing here."""
import itertools

import numpy as np
import pytest

from tests import plane_warp_ref as R
from tests import reduced_ref, warp_ref

pytestmark = pytest.mark.gpu

F32, U8, U16, U32 = np.float32, np.uint8, np.uint16, np.uint32
CODE = {"float32": 0, "float16": 1, "bfloat16": 2, "uint8": 3}  # DFX_PLANAR_F32 / _F16 / _BF16, DFX_WARP_U8
HOLDS = {"float32": U32, "float16": U16, "bfloat16": U16, "uint8": U8}  # the integer type that holds an element's bits
FILL = {U32: 0xA5A5A5A5, U16: 0xA5A5, U8: 0xA5}  # no NaN in any of the float types
BILINEAR = [(s, o) for s in R.FLOATS for o in R.FLOATS]
NEAREST = [(d, d) for d in ("uint8", "float16", "bfloat16", "float32")]
# (w, h) around the 256 x 4 workgroup and the 4-pixel quad, each with three channel counts: below, at and one beyond the
# channels of a 16-byte group for every element size; every count of {1, 2, 3, 4, 5, 7, 8, 9, 16, 17} occurs
SHAPES = {(1, 1): (1, 2, 17), (3, 2): (3, 4, 16), (5, 1): (5, 7, 8), (63, 3): (9, 1, 16), (64, 4): (2, 8, 17), (65, 5): (3, 4, 9),
          (255, 4): (1, 5, 16), (256, 4): (2, 7, 8), (257, 5): (4, 9, 17), (260, 9): (3, 8, 16), (97, 61): (1, 5, 17),
          (130, 97): (2, 4, 7)}
assert {c for cs in SHAPES.values() for c in cs} == {1, 2, 3, 4, 5, 7, 8, 9, 16, 17}


def _torch():
    import torch

    return torch


class Buf:
    """n items of p planes of h rows of roww elements in a device buffer of one of three layouts, the rest of it a fill:
    "dense"; "vector" (every base and stride a multiple of 16 elements, rows padded, gaps between planes and items); "offset"
    (the base one or three elements in, odd pitches and gaps).  k varies the paddings between the buffers of a call."""

    def __init__(self, n, p, h, roww, dtype, fill, layout, k=0, data=None):
        self.shape, self.dtype = (n, p, h, roww), np.dtype(dtype)
        if layout == "offset":
            lead, pitch = 1 + 2 * (k % 2), roww + 1 + 2 * (k % 2)
            plane = h * pitch + 1 + k % 3
            item = p * plane + 1 + 2 * (k % 3)
        elif layout == "vector":
            lead, pitch = 0, (roww + 15) // 16 * 16 + 16 * (1 + k % 2)
            plane = h * pitch + 16
            item = p * plane + 16
        else:
            lead, pitch, plane, item = 0, roww, h * roww, p * h * roww
        self.lead, self.pitch, self.plane, self.item = lead, pitch, plane, item
        self.host = np.full(lead + n * item + 64, fill, self.dtype)  # 64 elements of guard band behind the last item
        if data is not None:
            self.window(self.host)[...] = np.asarray(data).reshape(self.shape)
        self.dev = _torch().from_numpy(self.host.view(U8)).cuda()

    def window(self, flat):
        it = self.dtype.itemsize
        return np.lib.stride_tricks.as_strided(flat[self.lead:], self.shape, (self.item * it, self.plane * it, self.pitch * it, it))

    def ptr(self):
        return self.dev.data_ptr() + self.lead * self.dtype.itemsize

    def fill_with(self, flat):
        """Puts a host image of the whole buffer on the device (the garbage a keep call starts from)."""
        self.dev.copy_(_torch().from_numpy(flat.view(U8)))

    def read(self):
        return self.dev.cpu().numpy().view(self.dtype)


def _payload(rng, n, c, h, w, dtype, sample):
    """(n, c, h, w) source elements as the integers that hold their bits."""
    hold = HOLDS[dtype]
    if sample == "nearest":
        return rng.integers(0, 2 ** (8 * np.dtype(hold).itemsize), (n, c, h, w), dtype=np.uint64).astype(hold)
    v = (rng.standard_normal((n, c, h, w)) * 10.0 ** rng.integers(-3, 4, (n, c, 1, 1))).astype(F32)
    edge = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 1e-40, -1e-45, 65504.0, -65520.0, 6e-8, 3.3e38, -3.3e38, 1.0], F32)
    where = rng.random(v.shape) < 0.04
    v[where] = edge[rng.integers(0, len(edge), int(where.sum()))]
    bits = v.view(U32) if dtype == "float32" else R.stored(v, dtype)
    some = rng.random(v.shape) < 0.03  # random bit patterns among them: half subnormals, NaN payloads, extremes
    bits = bits.copy()
    bits[some] = rng.integers(0, 2 ** (8 * np.dtype(hold).itemsize), int(some.sum()), dtype=np.uint64).astype(hold)
    return bits


def _typed(bits, dtype):
    """The source as tests/plane_warp_ref.py takes it: float32 values, or the uint16 bits of a half type."""
    return bits.view(F32) if dtype == "float32" and bits.dtype == U32 else bits


def _flows(rng, n, h, w):
    f = np.ascontiguousarray(warp_ref.warp_flow(rng, n, h, w))
    for i in range(n):
        warp_ref.plant_specials(f[i])
    return f


class Scene:
    """n sources (n, c, h, w) of one dtype, their flows and masks, on the device in one buffer layout and in both memory
    layouts, with the reference's results cached per setting."""

    def __init__(self, eng, rng, n, c, h, w, src_dtype, sample, layout, flows=None, bits=None):
        self.eng, self.n, self.c, self.h, self.w, self.src_dtype, self.sample, self.layout = eng, n, c, h, w, src_dtype, sample, layout
        self.bits = _payload(rng, n, c, h, w, src_dtype, sample) if bits is None else bits
        self.flows = _flows(rng, n, h, w) if flows is None else flows
        self.occ = (rng.random((n, h, w)) < 0.25).astype(U8)
        hold = self.bits.dtype
        pad = {U32: 0x7FC00000, U16: 0x7E00, U8: 0xFF}[hold.type]  # NaN / 0xFF round the source
        self.src = {"chw": Buf(n, c, h, w, hold, pad, layout, 0, self.bits),
                    "hwc": Buf(n, 1, h, w * c, hold, pad, layout, 0, self.bits.transpose(0, 2, 3, 1))}
        self.dflow = Buf(n, 2, h, w, F32, np.nan, layout, 1, self.flows)
        self.docc = Buf(n, 1, h, w, U8, 1, layout, 3, self.occ)
        self.refs = {}

    def ref(self, out_dtype, border, with_occ):
        """(new (n, c, h, w) as held bits, take (n, h, w), valid (n, h, w)) of the reference."""
        key = (out_dtype, border, with_occ)
        if key not in self.refs:
            new, take, valid = [], [], []
            for i in range(self.n):
                src = self.bits[i].transpose(1, 2, 0)  # nearest: the held bits themselves
                occ = self.occ[i] if with_occ else None
                if self.sample == "bilinear":
                    s, t = R.bilinear(R.to_f32(_typed(src, self.src_dtype), self.src_dtype), self.flows[i], border)
                    e = R.stored(s, out_dtype)
                    e = e.view(U32) if out_dtype == "float32" else e
                else:
                    e, t = R.nearest(src, self.flows[i], border)
                new.append(e.transpose(2, 0, 1)), take.append(t), valid.append(R.valid_of(self.flows[i], occ))
            self.refs[key] = np.stack(new), np.stack(take), np.stack(valid)
        return self.refs[key]

    def check(self, mem, out_dtype, border="zero", keep=False, with_occ=False, outputs=("out", "valid"), k=0, tag=()):
        n, c, h, w = self.n, self.c, self.h, self.w
        hold = HOLDS[out_dtype]
        new, take, valid = self.ref(out_dtype, border, with_occ)
        out = Buf(n, c, h, w, hold, FILL[hold], self.layout, 4 + k) if mem == "chw" else Buf(n, 1, h, w * c, hold, FILL[hold], self.layout, 4 + k)
        dval = Buf(n, 1, h, w, U8, 0xA5, self.layout, 6 + k)
        want = out.host.copy()
        if keep:  # garbage the call must leave alone wherever a pixel is not valid
            want = np.random.default_rng(99).integers(0, 2 ** (8 * want.dtype.itemsize), want.shape, dtype=np.uint64).astype(hold)
            if out_dtype != "uint8":  # no NaN among the garbage: a kept element is compared bit for bit
                nan = np.isnan(want.view(F32)) if out_dtype == "float32" else reduced_ref.is_nan_bits(want, out_dtype)
                want[nan] = 0
            out.fill_with(want)
            mask = np.broadcast_to((valid != 0)[:, None], new.shape)
        else:
            new = np.where(take[:, None], new, hold(0))
            mask = np.ones(new.shape, bool)
        win = out.window(want)
        if mem == "hwc":
            new, mask = new.transpose(0, 2, 3, 1).reshape(win.shape), np.ascontiguousarray(mask.transpose(0, 2, 3, 1)).reshape(win.shape)
        if "out" in outputs:
            win[mask] = new[mask]
        want_valid = dval.host.copy()
        if "valid" in outputs:
            dval.window(want_valid)[...] = valid[:, None]
        src = self.src[mem]
        planar = mem == "chw"
        self.eng.warp_planes_device(
            src.ptr(), CODE[self.src_dtype], c, 1 if planar else 0, src.pitch, src.plane if planar else 0, src.item,
            self.dflow.ptr(), self.dflow.pitch, self.dflow.plane, self.dflow.item, n, R.BORDERS.index(border),
            R.SAMPLES.index(self.sample), int(keep), CODE[out_dtype], out.ptr() if "out" in outputs else None, out.pitch,
            out.plane if planar else 0, out.item, self.docc.ptr() if with_occ else None, self.docc.pitch, self.docc.item,
            dval.ptr() if "valid" in outputs else None, dval.pitch, dval.item)
        tag = (self.w, self.h, c, mem, self.sample, self.src_dtype, out_dtype, border, keep, with_occ, outputs, self.layout) + tuple(tag)
        got = out.read()
        if not R.same(got, want, out_dtype if self.sample == "bilinear" else None):
            bad = np.flatnonzero(got != want)
            raise AssertionError((tag, "out", len(bad), bad[:6], got[bad[:6]], want[bad[:6]]))
        assert np.array_equal(dval.read(), want_valid), (tag, "valid")
        return got

    def inputs_untouched(self):
        return all(np.array_equal(b.read().view(U8), b.host.view(U8)) for b in (self.src["chw"], self.src["hwc"], self.dflow, self.docc))


@pytest.fixture(scope="module")
def eng(dfx):
    with dfx.FlowEngine(260, 97, "farn") as e:
        yield e


@pytest.mark.parametrize("w,h", list(SHAPES))
def test_every_shape_and_channel_count_on_a_handle_resized(eng, w, h):
    eng.set_size(w, h)
    rng = np.random.default_rng(1000 * w + h)
    pairs = itertools.cycle([("bilinear",) + p for p in BILINEAR] + [("nearest",) + p for p in NEAREST])
    rest = itertools.cycle(itertools.product(R.BORDERS, (False, True), (False, True), (("out", "valid"), ("out",))))
    for c in SHAPES[(w, h)]:
        for layout in ("dense", "vector", "offset"):
            for _ in range(2):
                sample, sd, od = next(pairs)
                sc = Scene(eng, rng, 2, c, h, w, sd, sample, layout)
                for mem in ("chw", "hwc"):
                    border, keep, with_occ, outputs = next(rest)
                    sc.check(mem, od, border, keep, with_occ, outputs)
                assert sc.inputs_untouched()


@pytest.mark.parametrize("c", [3, 16])
@pytest.mark.parametrize("sample", R.SAMPLES)
def test_the_grid_of_settings(eng, sample, c):
    w, h = 97, 61
    eng.set_size(w, h)
    rng = np.random.default_rng(77 + c)
    calls = 0
    for sd in (R.FLOATS if sample == "bilinear" else [p[0] for p in NEAREST]):
        sc = Scene(eng, rng, 2, c, h, w, sd, sample, "vector")
        for od in (R.FLOATS if sample == "bilinear" else (sd,)):
            for mem, border, with_occ in itertools.product(("chw", "hwc"), R.BORDERS, (False, True)):
                for keep, outputs in ((False, ("out", "valid")), (False, ("out",)), (False, ("valid",)), (True, ("out", "valid")), (True, ("out",))):
                    if outputs == ("valid",) and od != sd:
                        continue  # nothing typed is stored
                    sc.check(mem, od, border, keep, with_occ, outputs)
                    calls += 1
        assert sc.inputs_untouched()
    assert calls >= 2 * 2 * 2 * 5 * 4


@pytest.mark.parametrize("mem", ["chw", "hwc"])
def test_the_wide_and_the_narrow_path_give_the_same_bits(eng, mem):
    w, h = 65, 9
    eng.set_size(w, h)
    for sample, sd, od in (("bilinear", "float32", "float32"), ("bilinear", "float16", "float16"), ("bilinear", "bfloat16", "float32"),
                           ("bilinear", "float32", "bfloat16"), ("nearest", "uint8", "uint8"), ("nearest", "float16", "float16"),
                           ("nearest", "float32", "float32")):
        rng = np.random.default_rng(5)
        first = Scene(eng, rng, 2, 16, h, w, sd, sample, "vector")
        rng = np.random.default_rng(5)
        second = Scene(eng, rng, 2, 16, h, w, sd, sample, "offset")
        assert np.array_equal(first.bits, second.bits)
        for keep in (False, True):
            a = first.check(mem, od, "clamp", keep, True)
            b = second.check(mem, od, "clamp", keep, True)
            hold = HOLDS[od]
            wa = Buf(2, 16, h, w, hold, 0, "vector", 4).window(a) if mem == "chw" else Buf(2, 1, h, w * 16, hold, 0, "vector", 4).window(a)
            wb = Buf(2, 16, h, w, hold, 0, "offset", 4).window(b) if mem == "chw" else Buf(2, 1, h, w * 16, hold, 0, "offset", 4).window(b)
            if not keep:  # every element is written: the very bits, a NaN's included
                assert np.array_equal(wa, wb), (sample, sd, od)


@pytest.mark.parametrize("w,h", [(97, 61), (13, 9), (5, 1)])
def test_landings_and_special_flow_values(eng, w, h):
    eng.set_size(w, h)
    rng = np.random.default_rng(531)
    base = _flows(rng, 2, h, w)
    whole = np.round(base)  # every landing exactly on an integer
    yy, xx = np.mgrid[0:h, 0:w].astype(F32)
    edge = np.stack([np.stack([F32(w - 1) - xx, F32(h - 1) - yy]),  # exactly the last column and row
                     np.stack([np.nextafter(F32(w - 1), F32(np.inf)) - xx, np.nextafter(F32(h - 1), F32(np.inf)) - yy])]).astype(F32)
    vals = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 1e-40, -1e-40, 0.5, -0.5, 1.5, 2.5, -0.0, 0.0], F32)
    special = vals[rng.integers(0, len(vals), base.shape)]
    bits = rng.integers(0, 2 ** 32, base.shape, dtype=np.uint64).astype(U32).view(F32)
    for name, fl in (("integers", whole), ("edges", edge), ("specials", special), ("bits", bits)):
        for sample, sd, od in (("bilinear", "float32", "float32"), ("bilinear", "float16", "float32"), ("nearest", "float16", "float16"),
                               ("nearest", "uint8", "uint8")):
            sc = Scene(eng, rng, 2, 3, h, w, sd, sample, "offset", flows=np.ascontiguousarray(fl))
            for mem, border, keep in (("chw", "zero", False), ("hwc", "clamp", False), ("chw", "clamp", True), ("hwc", "zero", True)):
                sc.check(mem, od, border, keep, with_occ=keep, tag=(name,))


def test_keep_beside_an_invalid_pixel_in_every_position_of_a_quad(eng):
    w, h = 16, 4
    eng.set_size(w, h)
    rng = np.random.default_rng(41)
    for sample, sd in (("bilinear", "float32"), ("bilinear", "float16"), ("nearest", "uint8"), ("nearest", "float32")):
        for layout in ("vector", "offset"):
            sc = Scene(eng, rng, 2, 2, h, w, sd, sample, layout, flows=np.zeros((2, 2, h, w), F32))
            yy, xx = np.mgrid[0:h, 0:w]
            sc.occ[:] = (xx % 4 == yy % 4).astype(U8)  # row y: the pixel at position y of every quad
            sc.docc = Buf(2, 1, h, w, U8, 1, layout, 3, sc.occ)
            for mem in ("chw", "hwc"):
                sc.check(mem, sd, "zero", True, True)
                sc.check(mem, sd, "zero", False, True)


@pytest.mark.parametrize("mem", ["chw", "hwc"])
def test_a_batch_larger_than_a_launch_holds(eng, mem):
    """n = 65537 images of 4 x 1, one channel: the launcher walks the batch in two launches."""
    torch = _torch()
    w, h, n = 4, 1, 65537
    eng.set_size(w, h)
    rng = np.random.default_rng(65537)
    src = rng.standard_normal((n, 1, h, w)).astype(F32)
    flows = np.zeros((n, 2, h, w), F32)
    flows[:, 0] = rng.uniform(-2.5, 2.5, (n, h, w)).astype(F32)
    # the reference, vectorised over the images: an image is one row, so with a vertical flow of 0 the n images stacked as
    # the rows of one image of height n sample as they do alone (ay = 0, and 0 * (b - t) adds nothing to a t that is not 0)
    s, take = R.bilinear(src[:, 0, 0, :, None], np.ascontiguousarray(flows[:, :, 0].transpose(1, 0, 2)), "zero")
    want = np.where(take, s[..., 0], F32(0)).reshape(n, 1, h, w)
    assert 0.3 < take.mean() < 0.9 and not (s == 0).any()
    d_src, d_fl = torch.from_numpy(src).cuda(), torch.from_numpy(flows).cuda()
    out = torch.full((n, 1, h, w), -7.0, device="cuda")
    valid = torch.full((n, h, w), 9, dtype=torch.uint8, device="cuda")
    eng.warp_planes_device(d_src.data_ptr(), 0, 1, 1 if mem == "chw" else 0, w, 0, w * h, d_fl.data_ptr(), w, w * h, 2 * w * h, n,
                           0, 0, 0, 0, out.data_ptr(), w, 0, w * h, None, 0, 0, valid.data_ptr(), w, w * h)
    assert np.array_equal(out.cpu().numpy().view(U32), want.view(U32))
    assert np.array_equal(valid.cpu().numpy(), take.reshape(n, h, w).astype(U8))


@pytest.mark.parametrize("stride_bytes", [2 ** 31 + 4096, 2 ** 32 + 4096])
@pytest.mark.parametrize("mem", ["chw", "hwc"])
def test_an_image_stride_beyond_2_and_4_gib(eng, mem, stride_bytes):
    """n = 2 images of 8 x 2 whose second image lies beyond 2^31 and beyond 2^32 bytes, source and output alike: only the two
    ends of the buffers are ever touched."""
    torch = _torch()
    w, h, c, n = 8, 2, 2, 2
    eng.set_size(w, h)
    rng = np.random.default_rng(stride_bytes % 1000)
    src = rng.standard_normal((n, c, h, w)).astype(F32)
    flows = _flows(rng, n, h, w)
    want, want_valid = R.warp_batch(src, flows, "chw", sample="bilinear", border="clamp")
    stride = stride_bytes // 4
    per = c * h * w
    big_src = torch.empty(stride + per, dtype=torch.float32, device="cuda")
    big_out = torch.empty(stride + per, dtype=torch.float32, device="cuda")
    lay = src if mem == "chw" else np.ascontiguousarray(src.transpose(0, 2, 3, 1))
    for i in range(n):
        big_src[i * stride:i * stride + per] = torch.from_numpy(lay[i].reshape(-1)).cuda()
        big_out[i * stride:i * stride + per] = -7.0
    d_fl = torch.from_numpy(flows).cuda()
    valid = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    planar = mem == "chw"
    eng.warp_planes_device(big_src.data_ptr(), 0, c, int(planar), w if planar else w * c, h * w if planar else 0, stride,
                           d_fl.data_ptr(), w, h * w, 2 * h * w, n, 1, 0, 0, 0, big_out.data_ptr(), w if planar else w * c,
                           h * w if planar else 0, stride, None, 0, 0, valid.data_ptr(), w, h * w)
    got = np.stack([big_out[i * stride:i * stride + per].cpu().numpy() for i in range(n)]).reshape(lay.shape)
    if not planar:
        got = got.transpose(0, 3, 1, 2)
    assert R.same(np.ascontiguousarray(got), want, "float32")
    assert np.array_equal(valid.cpu().numpy(), want_valid)


@pytest.mark.parametrize("which", ["src", "out"])
def test_a_plane_that_spans_more_than_4_gib(eng, which):
    """One image of 8 x 2 whose second row lies beyond 2^32 bytes, in the source or in the output: the planar kernel's form with
    64-bit lane offsets.  Only the two rows are ever touched."""
    torch = _torch()
    w, h = 8, 2
    eng.set_size(w, h)
    rng = np.random.default_rng(4)
    src = rng.standard_normal((1, 1, h, w)).astype(F32)
    flows = _flows(rng, 1, h, w)
    want, _ = R.warp_batch(src, flows, "chw", sample="bilinear", border="clamp")
    far = 2 ** 30 + 1024  # floats between the two rows
    pitch = {"src": (far, w), "out": (w, far)}[which]
    bufs = [torch.empty(p + w, dtype=torch.float32, device="cuda") for p in pitch]
    for y in range(h):
        bufs[0][y * pitch[0]:y * pitch[0] + w] = torch.from_numpy(src[0, 0, y]).cuda()
        bufs[1][y * pitch[1]:y * pitch[1] + w] = -7.0
    d_fl = torch.from_numpy(flows).cuda()
    eng.warp_planes_device(bufs[0].data_ptr(), 0, 1, 1, pitch[0], 0, h * pitch[0], d_fl.data_ptr(), w, h * w, 2 * h * w, 1, 1, 0, 0,
                           0, bufs[1].data_ptr(), pitch[1], 0, h * pitch[1])
    got = np.stack([bufs[1][y * pitch[1]:y * pitch[1] + w].cpu().numpy() for y in range(h)]).reshape(1, 1, h, w)
    assert R.same(got, want, "float32")


@pytest.mark.parametrize("form", ["gray", "chw", "hwc"])
def test_pictures_converted_to_float32_warp_as_the_8_bit_warp_does_on_the_device(dfx, form):
    torch = _torch()
    w, h, n = 97, 61, 2
    rng = np.random.default_rng(12)
    flows = torch.from_numpy(_flows(rng, n, h, w)).cuda()
    occ = torch.from_numpy((rng.random((n, h, w)) < 0.2).astype(U8)).cuda()
    shape = {"gray": (n, h, w), "chw": (n, 3, h, w), "hwc": (n, h, w, 3)}[form]
    img = torch.from_numpy(rng.integers(0, 256, shape, dtype=U8)).cuda()
    with dfx.FlowEngine(w, h, "farn") as eng:
        for border in R.BORDERS:
            want, want_valid = eng.warp_tensor(img, flows, border, torch.float32, occ=occ, want_valid=True)
            planes = img.float() if form != "gray" else img.float()[:, None]
            got, valid = eng.warp_planes_tensor(planes, flows, "bilinear", border, layout="hwc" if form == "hwc" else "chw", occ=occ,
                                                return_valid=True)
            assert torch.equal(got.reshape(want.shape).view(torch.int32), want.view(torch.int32))
            assert torch.equal(valid, want_valid)


def test_the_wrappers_agree_and_read_tensors_where_they_lie(dfx):
    torch = _torch()
    w, h, n, c = 33, 21, 2, 8
    rng = np.random.default_rng(3)
    src = rng.standard_normal((n, c, h, w)).astype(F32)
    labels = rng.integers(-2 ** 31, 2 ** 31, (n, c, h, w)).astype(np.int32)
    flows = _flows(rng, n, h, w)
    occ = (rng.random((n, h, w)) < 0.2).astype(U8)
    with dfx.FlowEngine(w, h, "tvl1") as eng:
        before, stats = eng.device_bytes(), bytes(eng.stats())
        seen = []
        raw = eng.warp_planes_device
        eng.warp_planes_device = lambda *a, **k: (seen.append(a[0]), raw(*a, **k))[1]
        t_flows, t_occ = torch.from_numpy(flows).cuda(), torch.from_numpy(occ).cuda()
        for sample, data, dt in (("bilinear", src, "float32"), ("nearest", labels, None)):
            want, want_valid = R.warp_batch(data, flows, "chw", occ=occ, sample=sample, border="clamp")
            a, va = eng.warp_planes(data, flows, sample, "clamp", occ=occ, return_valid=True)
            assert R.same(a, want, dt) and np.array_equal(va, want_valid)
            hwc = np.ascontiguousarray(data.transpose(0, 2, 3, 1))
            b = eng.warp_planes(hwc, flows, sample, "clamp", layout="hwc", occ=occ)
            assert R.same(np.ascontiguousarray(b.transpose(0, 3, 1, 2)), want, dt)
            t = torch.from_numpy(data).cuda()
            held = eng.device_bytes()
            for view in (t, t.contiguous(memory_format=torch.channels_last), torch.from_numpy(hwc).cuda().permute(0, 3, 1, 2)):
                seen.clear()
                g, vg = eng.warp_planes_tensor(view, t_flows, sample, "clamp", occ=t_occ, return_valid=True)
                assert seen == [view.data_ptr()], "the tensor was copied"
                assert g.shape == view.shape and (g.stride(1) == 1) == (view.stride(1) == 1)  # in the planes' memory layout
                assert R.same(g.cpu().numpy(), want, dt) and np.array_equal(vg.cpu().numpy(), want_valid)
            big = torch.zeros((n, c + 3, h + 2, w + 5), dtype=t.dtype, device="cuda")
            big[:, 1:c + 1, 1:h + 1, 2:w + 2] = t
            part = big[:, 1:c + 1, 1:h + 1, 2:w + 2]  # a slice of a larger tensor
            seen.clear()
            g = eng.warp_planes_tensor(part, t_flows, sample, "clamp", occ=t_occ)
            assert seen == [part.data_ptr()] and R.same(g.cpu().numpy(), want, dt)
            # keep: out is required, and what it held survives where a pixel is not valid
            fill = torch.full_like(t, 7)
            k = eng.warp_planes_tensor(t, t_flows, sample, "zero", "keep", occ=t_occ, out=fill)
            assert k is fill
            m = torch.from_numpy(want_valid != 0).cuda()[:, None].expand_as(t)
            assert bool((fill[~m] == 7).all()) and R.same(fill[m].cpu().numpy(), torch.from_numpy(want).cuda()[m].cpu().numpy(), dt)
            with pytest.raises(ValueError, match="needs out"):
                eng.warp_planes_tensor(t, t_flows, sample, invalid="keep")
            assert eng.device_bytes() == held, "the call allocated"
        half = eng.warp_planes_tensor(torch.from_numpy(src).cuda().half(), t_flows, dtype=torch.bfloat16)
        ref, _ = R.warp_batch(R.stored(src, "float16"), flows, "chw", sample="bilinear", src_dtype="float16", out_dtype="bfloat16")
        assert R.same(half.view(torch.int16).cpu().numpy().view(U16), ref, "bfloat16")
        with pytest.raises(ValueError, match='sample="nearest"'):
            eng.warp_planes_tensor(torch.from_numpy(labels).cuda(), t_flows)
        none = eng.warp_planes_tensor(torch.from_numpy(src).cuda()[:0], t_flows[:0], return_valid=True)
        assert none[0].shape == (0, c, h, w) and none[1].shape == (0, h, w)
        assert eng.device_bytes() == before and bytes(eng.stats()) == stats, "dfx_get_stats or dfx_device_bytes changed"


def test_every_refusal_returns_its_status_and_leaves_the_handle_usable(dfx):
    w, h, c = 33, 9, 4
    rng = np.random.default_rng(17)
    with dfx.FlowEngine(w, h, "tvl1") as eng:
        before, stats = eng.device_bytes(), bytes(eng.stats())
        for mem in ("chw", "hwc"):
            sc = Scene(eng, rng, 2, c, h, w, "float32", "bilinear", "vector")
            planar = mem == "chw"
            src = sc.src[mem]
            out = Buf(2, c, h, w, U32, FILL[U32], "vector", 4) if planar else Buf(2, 1, h, w * c, U32, FILL[U32], "vector", 4)
            dval = Buf(2, 1, h, w, U8, 0xA5, "vector", 6)
            names = ["d_src_ptr", "src_dtype", "channels", "layout", "src_pitch", "src_plane_stride", "src_image_stride", "d_flow_ptr",
                     "row_pitch_floats", "plane_stride_floats", "flow_stride_floats", "n", "border", "sample", "invalid", "out_dtype",
                     "d_out_ptr", "out_pitch", "out_plane_stride", "out_image_stride", "d_occ_ptr", "occ_pitch", "occ_stride",
                     "d_valid_ptr", "valid_pitch", "valid_stride"]
            good = dict(zip(names, [src.ptr(), 0, c, int(planar), src.pitch, src.plane if planar else 0, src.item, sc.dflow.ptr(),
                                    sc.dflow.pitch, sc.dflow.plane, sc.dflow.item, 2, 0, 0, 0, 0, out.ptr(), out.pitch,
                                    out.plane if planar else 0, out.item, sc.docc.ptr(), sc.docc.pitch, sc.docc.item, dval.ptr(),
                                    dval.pitch, dval.item]))
            row = w if planar else w * c
            refused = [dict(d_src_ptr=None), dict(d_flow_ptr=None), dict(d_out_ptr=None, d_valid_ptr=None), dict(n=-1),
                       dict(channels=0), dict(channels=-3), dict(layout=2), dict(layout=-1), dict(border=2), dict(border=-1),
                       dict(sample=2), dict(sample=-1), dict(invalid=2), dict(invalid=-1), dict(src_dtype=4), dict(src_dtype=-1),
                       dict(out_dtype=4), dict(out_dtype=-1), dict(src_dtype=3), dict(out_dtype=3),  # bilinear with 8-bit elements
                       dict(sample=1, out_dtype=1), dict(sample=1, src_dtype=3), dict(sample=1, src_dtype=1, out_dtype=2),
                       dict(invalid=1, d_out_ptr=None), dict(d_out_ptr=src.ptr()),
                       dict(src_pitch=row - 1), dict(src_image_stride=(c * src.plane if planar else h * src.pitch) - 1),
                       dict(out_pitch=row - 1), dict(out_image_stride=(c * out.plane if planar else h * out.pitch) - 1),
                       dict(row_pitch_floats=w - 1), dict(plane_stride_floats=h * sc.dflow.pitch - 1),
                       dict(flow_stride_floats=2 * sc.dflow.plane - 1), dict(occ_pitch=w - 1), dict(occ_stride=h * sc.docc.pitch - 1),
                       dict(valid_pitch=w - 1), dict(valid_stride=h * dval.pitch - 1)]
            if planar:
                refused += [dict(src_plane_stride=h * src.pitch - 1), dict(out_plane_stride=h * out.pitch - 1)]
            for over in refused:
                with pytest.raises(dfx.DfxError) as e:
                    eng.warp_planes_device(**{**good, **over})
                assert e.value.status == 1, over  # DFX_ERR_INVALID
                assert np.array_equal(out.read(), out.host) and np.array_equal(dval.read(), dval.host), (over, "a refused call wrote")
            assert eng._L.dfx_warp_planes_device(eng._h, None) == 1  # a NULL descriptor
            eng.warp_planes_device(**{**good, "n": 0, "d_src_ptr": None, "channels": 0, "layout": 9})  # n = 0: before anything else
            assert np.array_equal(out.read(), out.host)
            sc.check(mem, "float32", "clamp", False, True)  # the next valid call succeeds
        assert eng.device_bytes() == before and bytes(eng.stats()) == stats
    with dfx.FlowEngine(w, h, "frames") as eng:
        sc = Scene(eng, rng, 1, 1, h, w, "float32", "bilinear", "dense")
        with pytest.raises(dfx.DfxError) as e:
            sc.check("chw", "float32")
        assert e.value.status == 4  # DFX_ERR_UNSUPPORTED
