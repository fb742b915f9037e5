"""The Python binding's shared base, family by family: every bank class and its single object is created at the smallest size it
takes, fed, synchronised, asked for its counters, closed twice -- and made to fail: a unit index past the end must come back as
ERR_ARG with that family's own message (the base's _ck reads the family's last_error), a window table of the wrong length as
ERR_ARG before any create.  The families with a frames feed take three frames and count their batches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

UNITS = 2
BATCHES = 2
# three AdcDac frames of BATCHES batches each: Loss::update adds header.batches (byte 3 of the header) a frame (src/loss.rs:12)
RECEIVED = 3 * BATCHES

# name: (bank, single, feed, size, second key of stats_read, frames entry of one unit)
#   feed: what process takes a unit -- "real" x, "pair" x, y, "group" [x] * m, "iq" z, "iqpair" za, zb
#   size: the name of the family's *_supported(n), or the smallest n its create documents (include/psdcascade.h)
FAMILIES = {
    "psd": ("PsdCascadeBank", "PsdCascade", "real", 16, None, ()),
    "csd": ("CsdCascadeBank", "CsdCascade", "pair", 64, "pairs_in", (0, 1)),
    "csm": ("CsmCascadeBank", "CsmCascade", "group", "csm_supported", "sample_times_in", (0, 1)),
    "zoom": ("ZoomCascadeBank", "ZoomCascade", "real", 64, "samples_in", 2),
    "sk": ("SkCascadeBank", "SkCascade", "real", "sk_supported", "samples_in", None),
    "iq": ("IqCascadeBank", "IqCascade", "iq", 64, "samples_in", (2, 3)),
    "zsk": ("ZoomSkCascadeBank", "ZoomSkCascade", "real", "zoom_sk_supported", "samples_in", None),
    "iqsk": ("IqSkCascadeBank", "IqSkCascade", "iq", "zoom_sk_supported", "samples_in", None),
    "wf": ("WaterfallCascadeBank", "WaterfallCascade", "real", "waterfall_supported", "samples_in", None),
    "zwf": ("ZoomWaterfallCascadeBank", "ZoomWaterfallCascade", "real", "zoom_waterfall_supported", "samples_in", None),
    "zampm": ("ZoomAmPmCascadeBank", "ZoomAmPmCascade", "real", "zoom_ampm_supported", "samples_in", None),
    "iqampm": ("IqAmPmCascadeBank", "IqAmPmCascade", "iq", "zoom_ampm_supported", "samples_in", None),
    "zcsd": ("ZoomCsdCascadeBank", "ZoomCsdCascade", "pair", "zcsd_supported", "pairs_in", (0, 1)),
    "iqcsd": ("IqCsdCascadeBank", "IqCsdCascade", "iqpair", "iqcsd_supported", "pairs_in", ((0, 1), (2, 3))),
    "zxampm": ("ZoomAmPmCsdCascadeBank", "ZoomAmPmCsdCascade", "pair", "zoom_ampm_cross_supported", "pairs_in", None),
    "iqxampm": ("IqAmPmCsdCascadeBank", "IqAmPmCsdCascade", "iqpair", "zoom_ampm_cross_supported", "pairs_in", None),
}
M = 2  # channels of a matrix group


def smallest(pkg, name):
    size = FAMILIES[name][3]
    if isinstance(size, int):
        return size
    ok = getattr(pkg, size)
    return next(n for n in (16, 32, 64, 128, 256) if (ok(n, M) if name == "csm" else ok(n)))


def units_of(name):
    return 4 if name == "psd" else UNITS  # psdc_process_frames sends trace i to channel i: it needs four channels


def make(pkg, name, single, n, window=None):
    cls = getattr(pkg, FAMILIES[name][1 if single else 0])
    args = (n, M) if name == "csm" else (n,)
    if not single:
        args += (units_of(name),)
    return cls(*args) if window is None else cls(*args, window=window)


def streams(pkg, name, n, seed):
    """what process takes for one unit, from 8 n + 37 seeded samples a stream"""
    ln = 8 * n + 37
    x = [pkg.noise_host(ln, seed + k) for k in range(4)]
    return {"real": (x[0],), "pair": (x[0], x[1]), "group": ([x[0], x[1]],), "iq": ((x[0] + 1j * x[1]).astype(np.complex64),),
            "iqpair": ((x[0] + 1j * x[1]).astype(np.complex64), (x[2] + 1j * x[3]).astype(np.complex64))}[FAMILIES[name][2]]


@pytest.fixture(scope="module")
def frames(pkg):
    """three valid AdcDac frames, made once"""
    rng = np.random.default_rng(11)
    words = rng.integers(-2000, 2000, (4, 8 * BATCHES * 3)).astype(np.int16)
    data, fs = pkg.make_adcdac_frames(words, BATCHES, seq0=5)
    assert len(data) == 3 * fs
    return data, fs


@pytest.mark.parametrize("single", [False, True], ids=["bank", "single"])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_lifecycle(pkg, gpu_required, frames, name, single):
    key, entry = FAMILIES[name][4], FAMILIES[name][5]
    n = smallest(pkg, name)
    units = 1 if single else units_of(name)
    obj = make(pkg, name, single, n)
    for u in range(units):
        obj.process(*(() if single else (u,)), *streams(pkg, name, n, 100 * u + 1))
    obj.sync()
    assert all(obj.num_stages(*(() if single else (u,))) >= 1 for u in range(units))
    if key is not None:
        st = obj.stats_read()
        assert sorted(st) == sorted(["launches", key]) and st["launches"] >= 1, st
    if not single:
        with pytest.raises(pkg.PsdError) as e:
            obj.num_stages(units)
        assert e.value.code == pkg.ERR_ARG and type(e.value) is pkg.PsdError
        msg = str(e.value).split(": ", 1)[1]
        assert msg, "the family's last_error gave no message"
    if entry is not None and (name != "psd" or not single):
        data, fs = frames
        got = obj.process_frames(data, fs, *(() if name == "psd" else (entry if single else [entry] * units,)))
        assert got == 3
        assert obj.loss()["received"] == RECEIVED
    obj.close()
    obj.close()
    assert obj._b._h is None if single else obj._h is None


@pytest.mark.parametrize("single", [False, True], ids=["bank", "single"])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_window_table_of_the_wrong_length(pkg, gpu_required, name, single):
    n = smallest(pkg, name)
    table = pkg.WindowTable.hann(2 * n)
    with pytest.raises(pkg.PsdError) as e:
        make(pkg, name, single, n, window=table)
    assert e.value.code == pkg.ERR_ARG and "window table length != n" in str(e.value)
