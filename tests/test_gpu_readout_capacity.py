"""The capacity and size-query paths of the host read-outs of the cross-spectral runtime (csrc/cross_runtime.cpp), through the C ABI.

The Python binding always passes a capacity that is large enough, so its tests never reach these paths.  Here every one of the
fifteen families gets one object at n = 64 with one unit fed 64 * 8 * 8 + 64 samples (three stages), and every stitched read-out
it has is called

  * with every output NULL (the size query): PSDC_OK, len > 0 and n_breaks > 0;
  * with cap = len and breaks_cap = n_breaks: PSDC_OK, and every value and Break bit-equal to the same call with the binding's
    generous capacity (stages x bins);
  * with cap = len - 1, and with breaks_cap = n_breaks - 1: PSDC_ERR_CAPACITY, with a text that names the function (a pair or a
    matrix object stitches through the public psdc_cross_stitch / psdc_csm_stitch, whose name its text carries);
  * in all of these with guard elements behind `cap` elements of every output, which stay as they were;
  * and, where it writes f64 (SK, the sidebands) into more than one output, with one output alone, which then holds the same
    values as when all are given.

The two waterfall families have no stitched read-out: their stage_rows takes the place of it, with max_rows as the capacity (the
rows a call returns are the newest min(max_rows, valid)), and their stage read-outs name the function when the stage is out of
range, as every family's do (one stage lookup serves them all).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, BINS = 64, 33
FED = 64 * 8 * 8 + 64
HANN = 1
GUARD = 7
F32, F64 = np.float32, np.float64

# family: prefix, the counts create takes between the window and the device, carrier ("", "unit", "side"), streams a feed takes,
# and its stitched read-outs: (function, [(dtype, elements a unit of capacity)], name in a capacity error's text)
FAMILIES = [
    ("psdc_cross", (1,), "", 2, [("psdc_cross_csd", [(F32, 1), (F32, 1), (F32, 2)], "psdc_cross_stitch")]),
    ("psdc_csm", (3, 1), "", 3, [("psdc_csm_csd", [(F32, 9)], "psdc_csm_stitch")]),
    ("psdc_zoom", (1,), "unit", 1, [("psdc_zoom_psd", [(F32, 1)] * 2, None)]),
    ("psdc_iq", (1,), "unit", 2, [("psdc_iq_psd", [(F32, 1)] * 2, None)]),
    ("psdc_zcsd", (1,), "side", 2, [("psdc_zcsd_csd", [(F32, 1)] * 4 + [(F32, 2)] * 2, None)]),
    ("psdc_iqcsd", (1,), "side", 4, [("psdc_iqcsd_csd", [(F32, 1)] * 4 + [(F32, 2)] * 2, None)]),
    ("psdc_sk", (1,), "", 1, [("psdc_sk_psd", [(F32, 1)], None), ("psdc_sk_sk", [(F64, 1)], None)]),
    ("psdc_zsk", (1,), "unit", 1, [("psdc_zsk_psd", [(F32, 1)] * 2, None), ("psdc_zsk_sk", [(F64, 1)] * 2, None)]),
    ("psdc_iqsk", (1,), "unit", 2, [("psdc_iqsk_psd", [(F32, 1)] * 2, None), ("psdc_iqsk_sk", [(F64, 1)] * 2, None)]),
    ("psdc_zampm", (1,), "unit", 1, [("psdc_zampm_psd", [(F32, 1)] * 2, None), ("psdc_zampm_sidebands", [(F64, 1)] * 4, None)]),
    ("psdc_iqampm", (1,), "unit", 2, [("psdc_iqampm_psd", [(F32, 1)] * 2, None), ("psdc_iqampm_sidebands", [(F64, 1)] * 4, None)]),
    ("psdc_zxampm", (1,), "side", 2, [("psdc_zxampm_sidebands", [(F64, 12)], None)]),
    ("psdc_iqxampm", (1,), "side", 4, [("psdc_iqxampm_sidebands", [(F64, 12)], None)]),
    ("psdc_wf", (1, 4, 3), "", 1, []),
    ("psdc_zwf", (1, 4, 3), "unit", 1, []),
]


def _ptr(a):
    if a is None:
        return None
    return a.ctypes.data_as(C.POINTER(C.c_float if a.dtype == F32 else C.c_double))


def _marked(dtype, elems):
    """An output of `elems` elements and GUARD more, every byte 0xCD"""
    return np.frombuffer(bytes([0xCD]) * (np.dtype(dtype).itemsize * (elems + GUARD)), dtype=dtype).copy()


def _guard_intact(a, elems):
    return a[elems:].tobytes() == bytes([0xCD]) * (a.itemsize * GUARD)


class Unit:
    """One object of a family with its unit 0 fed"""

    def __init__(self, pkg, fam):
        self.pkg, self.L = pkg, pkg.lib()
        self.pre, counts, carrier, streams, self.reads = fam
        self.h = getattr(self.L, self.pre + "_create")(N, HANN, *counts, 0)
        assert self.h, self.err(None)
        if carrier == "unit":
            assert self.fn("set_carrier")(self.h, 0, int(0.19 * 2 ** 64), 12345) == 0, self.err()
        elif carrier == "side":
            for side in (0, 1):
                assert self.fn("set_carrier")(self.h, 0, side, int((0.19 + 0.02 * side) * 2 ** 64), 12345 + side) == 0, self.err()
        rng = np.random.default_rng(20261021)
        self.x = [rng.standard_normal(FED).astype(F32) for _ in range(streams)]
        if self.pre == "psdc_csm":
            arr = (C.c_void_p * streams)(*[x.ctypes.data for x in self.x])
            rc = self.fn("process")(self.h, 0, arr, FED)
        else:
            rc = self.fn("process")(self.h, 0, *[_ptr(x) for x in self.x], FED)
        assert rc == 0, self.err()
        self.ns = self.fn("num_stages")(self.h, 0)
        assert self.ns == 3, self.err()

    def fn(self, name):
        return getattr(self.L, self.pre + "_" + name)

    def err(self, h="own"):
        return self.fn("last_error")(self.h if h == "own" else None).decode()

    def close(self):
        self.fn("destroy")(self.h)

    def stitched(self, fname, outs, cap, given=None, breaks_cap=None):
        """One call: outputs `given` (indices; None: all) of capacity cap.  -> rc, len, n_breaks, arrays (None where not given), breaks"""
        given = range(len(outs)) if given is None else given
        arrs = [_marked(dt, per * cap) if i in given else None for i, (dt, per) in enumerate(outs)]
        nbc = 16 if breaks_cap is None else breaks_cap
        br = (self.pkg._CBreak * (nbc + 1))()
        C.memset(br, 0xCD, C.sizeof(br))
        ln, nb = C.c_size_t(0xCDCD), C.c_size_t(0xCDCD)
        rc = getattr(self.L, fname)(self.h, 0, 0, 1, 0, *[_ptr(a) for a in arrs], cap, C.byref(ln), br, nbc, C.byref(nb))
        for a, (dt, per) in zip(arrs, outs):
            assert a is None or _guard_intact(a, per * cap), f"{fname}: cap {cap}: written behind the output's capacity"
        assert bytes(br)[C.sizeof(self.pkg._CBreak) * nbc:] == bytes([0xCD]) * C.sizeof(self.pkg._CBreak), f"{fname}: written behind breaks_cap"
        return rc, ln.value, nb.value, arrs, bytes(br)[:C.sizeof(self.pkg._CBreak) * min(nb.value, nbc)] if rc == 0 else b""


@pytest.fixture(scope="module", params=FAMILIES, ids=[f[0] for f in FAMILIES])
def unit(request, pkg, gpu_required):
    u = Unit(pkg, request.param)
    yield u
    u.close()


def _stitched_capacities(unit):
    pkg, L = unit.pkg, unit.L
    for fname, outs, err_name in unit.reads:
        err_name = err_name or fname
        # the size query
        ln, nb = C.c_size_t(0), C.c_size_t(0)
        rc = getattr(L, fname)(unit.h, 0, 0, 1, 0, *[None] * len(outs), 0, C.byref(ln), None, 0, C.byref(nb))
        assert rc == 0 and ln.value > 0 and nb.value > 0, (fname, rc, ln.value, nb.value, unit.err())
        ln, nb = ln.value, nb.value
        # the binding's generous capacity, then the exact ones: the same bits
        rc_g, ln_g, nb_g, big, br_g = unit.stitched(fname, outs, unit.ns * BINS)
        assert (rc_g, ln_g, nb_g) == (0, ln, nb), (fname, rc_g, ln_g, nb_g, unit.err())
        rc_e, ln_e, nb_e, exact, br_e = unit.stitched(fname, outs, ln, breaks_cap=nb)
        assert (rc_e, ln_e, nb_e) == (0, ln, nb), (fname, rc_e, ln_e, nb_e, unit.err())
        assert br_e == br_g, f"{fname}: the Breaks differ with breaks_cap = n_breaks"
        for a, b, (dt, per) in zip(exact, big, outs):
            rows = per if per > 2 else 1  # (per > 2: that many rows one behind the other, `cap` elements apart)
            width = per // rows
            for r in range(rows):
                ea, eb = a[r * width * ln:(r + 1) * width * ln], b[r * width * unit.ns * BINS:r * width * unit.ns * BINS + width * ln]
                assert ea.tobytes() == eb.tobytes(), f"{fname}: row {r} differs between cap = len and the generous capacity"
        # too small
        rc, _, _, _, _ = unit.stitched(fname, outs, ln - 1)
        assert rc == pkg.ERR_CAPACITY and unit.err().startswith(err_name + ":"), (fname, rc, unit.err())
        rc, _, _, _, _ = unit.stitched(fname, outs, unit.ns * BINS, breaks_cap=nb - 1)
        assert rc == pkg.ERR_CAPACITY and unit.err().startswith(err_name + ":"), (fname, rc, unit.err())
        # an f64 read-out with one output alone
        if outs[0][0] == F64 and len(outs) > 1:
            for i in (0, len(outs) - 1):
                rc, ln_1, _, one, _ = unit.stitched(fname, outs, ln, given=[i])
                assert rc == 0 and ln_1 == ln, (fname, i, rc, unit.err())
                assert one[i].tobytes() == exact[i].tobytes(), f"{fname}: output {i} alone differs from output {i} among all"


def _stage_out_of_range(unit):
    """every family's stage read-outs go through one lookup of the drained stage: stage = number of stages is refused by name"""
    st = unit.pkg._CStageStat()
    wf = unit.pre in ("psdc_wf", "psdc_zwf")
    name = {"psdc_cross": "stage_spectra", "psdc_csm": "stage_spectra", "psdc_zoom": "stage_spectra", "psdc_iq": "stage_spectra",
            "psdc_zcsd": "stage_spectra", "psdc_iqcsd": "stage_spectra", "psdc_sk": "stage_moments", "psdc_zsk": "stage_moments",
            "psdc_iqsk": "stage_moments"}.get(unit.pre, "stage_blocks" if wf else "stage_rows")
    f = unit.fn(name)
    nargs = len(f.argtypes)
    if wf:
        rc = f(unit.h, 0, unit.ns, C.byref(unit.pkg._CWfBlocks()))
    else:
        rc = f(unit.h, 0, unit.ns, C.byref(st), *[None] * (nargs - 4))
    assert rc == unit.pkg.ERR_ARG, (rc, unit.err())
    assert unit.err() == f"{unit.pre}_{name}: stage {unit.ns} out of range ({unit.ns} stages)"


def _waterfall_capacities(unit):
    """stage_rows of the waterfalls: max_rows is the capacity.  The rows of a call with max_rows = rows_valid are those of a generous
    call, fewer rows are the newest ones, nothing is written behind max_rows rows, and a row set alone holds what it holds among all"""
    nsets = 2 if unit.pre == "psdc_wf" else 4
    blocks = unit.pkg._CWfBlocks()
    assert unit.fn("stage_blocks")(unit.h, 0, 0, C.byref(blocks)) == 0, unit.err()
    valid = blocks.rows_valid
    assert valid == 3  # (the ring's depth: stage 0 has seen many more blocks)

    def rows(max_rows, given=None):
        given = range(nsets) if given is None else given
        idx, counts, n_rows = np.zeros(max_rows, np.uint64), np.zeros(max_rows, np.uint32), C.c_uint32(0xCDCD)
        arrs = [_marked(F64, max_rows * BINS) if i in given else None for i in range(nsets)]
        rc = unit.fn("stage_rows")(unit.h, 0, 0, max_rows, idx.ctypes.data_as(C.POINTER(C.c_uint64)), counts.ctypes.data_as(C.POINTER(C.c_uint32)),
                                   *[_ptr(a) for a in arrs], C.byref(n_rows))
        assert rc == 0, unit.err()
        for a in arrs:
            assert a is None or _guard_intact(a, max_rows * BINS), f"max_rows {max_rows}: written behind the rows' capacity"
        return n_rows.value, idx, arrs

    n_big, idx_big, big = rows(8)
    assert n_big == valid
    n_exact, idx_exact, exact = rows(valid)
    assert n_exact == valid and np.array_equal(idx_exact, idx_big[:valid])
    n_two, idx_two, two = rows(valid - 1)
    assert n_two == valid - 1 and np.array_equal(idx_two, idx_big[1:valid])
    for i in range(nsets):
        assert exact[i][:valid * BINS].tobytes() == big[i][:valid * BINS].tobytes(), f"row set {i} differs with max_rows = rows_valid"
        assert two[i][:(valid - 1) * BINS].tobytes() == big[i][BINS:valid * BINS].tobytes(), f"row set {i}: fewer rows are not the newest"
    _, _, last = rows(valid, given=[nsets - 1])
    assert last[nsets - 1].tobytes() == exact[nsets - 1].tobytes(), "the last row set alone differs from the same among all"


def test_readout_capacities(unit):
    """once a family: its stitched read-outs (the waterfalls: their stage_rows) at absent, exact and too small capacities, and its
    stage read-out at a stage that is not there"""
    if unit.reads:
        _stitched_capacities(unit)
    else:
        _waterfall_capacities(unit)
    _stage_out_of_range(unit)
