"""The forward-backward check on the device (dfx_fb_check_device, denseflow_amd/csrc/fb_check_kernels.hip) against its NumPy
reference (tests/fb_check_ref.py): masks with np.array_equal, err planes as bit patterns.  Sizes are the smallest at which
the kernel can go wrong — one pixel, a row shorter than a lane's four pixels, odd widths with a ragged tail, several 4-row
workgroups, and 261 x 5 for a second 256-pixel workgroup column — in every layout that selects another access width: dense,
unaligned (single elements), 16-byte aligned (16-byte loads of F, 4-byte mask stores, 16-byte err stores)."""
import numpy as np
import pytest

from tests import fb_check_ref as R
from tests.devmem import DevBuf

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = [(1, 1), (3, 2), (65, 17), (97, 61), (130, 97), (261, 5)]
GUARD = 64            # elements in front of and behind every output buffer
OCC_FILL, ERR_FILL = 0xA5, F32(-777.25)

_case_cache = {}


ALPHAS = [(R.ALPHA1, R.ALPHA2), (1.0, 0.5)]  # the defaults; and one that splits random flows about evenly: 2 F.s <= alpha2


def _case(w, h, n):
    """Flows and references (one per ALPHAS) of one (size, n), computed once and never changed: smooth fields of magnitude up
    to 1.5 W (a large share leaves the frame), the special values planted in the last pair."""
    key = (w, h, n)
    if key not in _case_cache:
        rng = np.random.default_rng(1000 * w + 10 * h + n)
        fwd, bwd = R.smooth_flow(rng, n, h, w, 1.5 * w), R.smooth_flow(rng, n, h, w, 1.5 * w)
        R.plant_specials(fwd[-1], bwd[-1])
        refs = [R.fb_check_batch(fwd, bwd, a1, a2) for a1, a2 in ALPHAS]
        for a in [fwd, bwd] + [x for r in refs for x in r]:
            a.setflags(write=False)
        _case_cache[key] = (fwd, bwd, refs)
    return _case_cache[key]


def _up4(v):
    return (v + 3) // 4 * 4


def _layouts(w, h):
    """name -> (flow lead floats, row pitch, plane stride, flow stride, mask lead bytes, mask pitch, mask stride,
    err lead floats, err pitch, err stride)."""
    p3 = w + 3
    p4 = _up4(w) + 4
    return {
        "dense": (0, w, h * w, 2 * h * w, 0, w, h * w, 0, w, h * w),
        # a base one float in, odd pitches: every access is a single element
        "scalar": (1, p3, h * p3 + 5, 2 * (h * p3 + 5) + 7, 1, w + 1, h * (w + 1) + 3, 1, p3, h * p3 + 1),
        # everything a multiple of 4 floats / 4 bytes from a 16-byte-aligned base: the wide accesses
        "vector": (0, p4, h * p4 + 8, 2 * (h * p4 + 8) + 12, 0, _up4(w), h * _up4(w) + 4, 0, p4, h * p4 + 4),
    }


def _pack(flows, lead, pitch, plane, stride):
    """(n, 2, H, W) flows in a padded buffer; the padding is NaN, so a read of it would show in the result."""
    n, _, h, w = flows.shape
    buf = np.full(lead + n * stride + 4, np.nan, F32)
    for i in range(n):
        for p in range(2):
            o = lead + i * stride + p * plane
            buf[o:o + h * pitch].reshape(h, pitch)[:, :w] = flows[i, p]
    return buf


def _windows(buf, n, h, w, lead, pitch, stride):
    """(the n windows of a padded output buffer, a mask of everything outside them)."""
    outside = np.ones(buf.shape, bool)
    wins = []
    for i in range(n):
        o = GUARD + lead + i * stride
        wins.append(buf[o:o + h * pitch].reshape(h, pitch)[:, :w].copy())
        outside[o:o + h * pitch].reshape(h, pitch)[:, :w] = False
    return np.stack(wins), outside


def _run(eng, fwd, bwd, layout, want_err, a1=R.ALPHA1, a2=R.ALPHA2):
    n, _, h, w = fwd.shape
    fl, rp, ps, fs, ol, op, os_, el, ep, es = layout
    occ_host = np.full(2 * GUARD + ol + n * os_, OCC_FILL, np.uint8)
    err_host = np.full(2 * GUARD + el + n * es, ERR_FILL, F32)
    with DevBuf(eng, init=_pack(fwd, fl, rp, ps, fs)) as d_f, DevBuf(eng, init=_pack(bwd, fl, rp, ps, fs)) as d_b, \
            DevBuf(eng, init=occ_host) as d_occ, DevBuf(eng, init=err_host) as d_err:
        eng.fb_check_device(d_f.ptr(4 * fl), d_b.ptr(4 * fl), rp, ps, fs, n, a1, a2, d_occ.ptr(GUARD + ol), op, os_,
                            d_err.ptr(4 * (GUARD + el)) if want_err else None, ep, es)
        occ_buf, err_buf = d_occ.get(np.uint8), d_err.get(F32)
    occ, occ_out = _windows(occ_buf, n, h, w, ol, op, os_)
    err, err_out = _windows(err_buf, n, h, w, el, ep, es)
    assert np.all(occ_buf[occ_out] == OCC_FILL), "a mask byte outside the W x H windows was written"
    if want_err:
        assert np.all(err_buf[err_out] == ERR_FILL), "an err float outside the W x H windows was written"
    else:
        assert np.all(err_buf == ERR_FILL), "err planes were written without being asked for"
    return occ, (err if want_err else None)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("w,h", SIZES)
def test_the_device_check_equals_the_reference_in_every_layout(dfx, w, h, n):
    fwd, bwd, refs = _case(w, h, n)
    outside = np.stack([R.out_of_frame(f) for f in fwd])
    if w * h >= 8:  # the taps are really sampled, and the second pair of alphas makes the comparison go both ways
        assert (~outside).sum() >= 8 and 0.2 < refs[1][0][~outside].mean() < 0.8
    with dfx.FlowEngine(w, h, "farn") as eng:
        for name, layout in _layouts(w, h).items():
            for want_err in (True, False):
                for (a1, a2), (occ_ref, err_ref) in zip(ALPHAS, refs):
                    occ, err = _run(eng, fwd, bwd, layout, want_err, a1, a2)
                    assert np.array_equal(occ, occ_ref), (name, want_err, a1)
                    if want_err:
                        bad = err.view(np.uint32) != err_ref.view(np.uint32)
                        assert not bad.any(), (name, int(bad.sum()), err[bad][:4], err_ref[bad][:4])
                        assert np.all(np.isposinf(err[outside]))
    print(f"{w}x{h} n={n}: out of frame {outside.mean():.3f}, occluded {refs[0][0].mean():.3f} / {refs[1][0].mean():.3f}")


@pytest.mark.parametrize("algo", ["tvl1", "brox"])
def test_numpy_wrapper_on_every_flow_handle(dfx, algo):
    w, h, n = 65, 17, 3
    fwd, bwd, refs = _case(w, h, n)
    occ_ref, err_ref = refs[0]
    with dfx.FlowEngine(w, h, algo) as eng:
        occ, err = eng.fb_check(fwd, bwd, R.ALPHA1, R.ALPHA2, want_err=True)
        only = eng.fb_check(fwd, bwd, R.ALPHA1, R.ALPHA2)
        other = eng.fb_check(fwd, bwd, 0.3, 2.0)
    assert occ.dtype == np.uint8 and occ.shape == (n, h, w) and err.dtype == F32
    assert np.array_equal(occ, occ_ref) and np.array_equal(only, occ_ref)
    assert np.array_equal(err.view(np.uint32), err_ref.view(np.uint32))
    assert np.array_equal(other, R.fb_check_batch(fwd, bwd, 0.3, 2.0)[0])


@pytest.mark.parametrize("layout", ["scalar", "vector"])
def test_the_threshold_edge(dfx, layout):
    w, h = 65, 17
    d = F32(1.3)
    fwd, bwd = np.zeros((1, 2, h, w), F32), np.zeros((1, 2, h, w), F32)
    fwd[0, 0] = d
    inside = ~R.out_of_frame(fwd[0])
    at = F32(d * d)
    below = np.nextafter(at, F32(0))
    with dfx.FlowEngine(w, h, "farn") as eng:
        occ_at, err = _run(eng, fwd, bwd, _layouts(w, h)[layout], True, 0.0, float(at))
        occ_below, _ = _run(eng, fwd, bwd, _layouts(w, h)[layout], False, 0.0, float(below))
    assert np.all(err[0][inside] == at)
    assert not occ_at[0][inside].any() and occ_at[0][~inside].all()   # err <= thr holds with equality
    assert occ_below[0].all()                                           # one ulp below: occluded
    assert np.array_equal(occ_at[0], R.fb_check(fwd[0], bwd[0], 0.0, at)[0])
    assert np.array_equal(occ_below[0], R.fb_check(fwd[0], bwd[0], 0.0, below)[0])


def test_every_refusal_returns_its_status_and_leaves_the_handle_usable(dfx):
    w, h, n = 65, 17, 3
    fwd, bwd, refs = _case(w, h, n)
    occ_ref = refs[0][0]
    fl, rp, ps, fs, ol, op, os_, el, ep, es = _layouts(w, h)["dense"]
    with dfx.FlowEngine(w, h, "tvl1") as eng:
        with DevBuf(eng, init=fwd) as d_f, DevBuf(eng, init=bwd) as d_b, \
                DevBuf(eng, init=np.full(n * h * w, OCC_FILL, np.uint8)) as d_occ, DevBuf(eng, 4 * n * h * w) as d_err:
            good = dict(f=d_f.ptr(), b=d_b.ptr(), rp=rp, ps=ps, fs=fs, n=n, a1=R.ALPHA1, a2=R.ALPHA2, occ=d_occ.ptr(), op=op,
                        os=os_, err=d_err.ptr(), ep=ep, es=es)

            def call(**kw):
                a = dict(good, **kw)
                eng.fb_check_device(a["f"], a["b"], a["rp"], a["ps"], a["fs"], a["n"], a["a1"], a["a2"], a["occ"], a["op"],
                                    a["os"], a["err"], a["ep"], a["es"])

            refused = [dict(f=None), dict(b=None), dict(occ=None), dict(n=-1), dict(rp=w - 1), dict(ps=rp * h - 1),
                       dict(fs=2 * ps - 1), dict(op=w - 1), dict(os=op * h - 1), dict(ep=w - 1), dict(es=ep * h - 1),
                       dict(a1=float("nan")), dict(a1=float("inf")), dict(a1=-0.01), dict(a2=float("nan")),
                       dict(a2=float("inf")), dict(a2=-1e-6)]
            for kw in refused:
                with pytest.raises(dfx.DfxError) as e:
                    call(**kw)
                assert e.value.status == 1, kw
            assert np.all(d_occ.get() == OCC_FILL), "a refused call wrote"
            call(n=0)  # DFX_OK, launches nothing
            call(n=0, f=None, b=None, occ=None)
            assert np.all(d_occ.get() == OCC_FILL), "n = 0 wrote"
            call(err=None, ep=0, es=0)  # without err planes their strides are not looked at
            assert np.array_equal(d_occ.get().reshape(n, h, w), occ_ref), "the handle is not usable after the refusals"
    with dfx.FlowEngine(w, h, "frames") as eng:
        with DevBuf(eng, init=fwd) as d_f, DevBuf(eng, n * h * w) as d_occ:
            with pytest.raises(dfx.DfxError) as e:
                eng.fb_check_device(d_f.ptr(), d_f.ptr(), rp, ps, fs, n, R.ALPHA1, R.ALPHA2, d_occ.ptr(), op, os_)
            assert e.value.status == 4
