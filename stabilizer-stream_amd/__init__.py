"""MI355X-native cascaded PSD estimator -- Python mirror of the reference surface.

Thin ctypes layer over the C ABI in include/psdcascade.h (libpsdcascade.so, HIP
kernels for gfx950).  Class and method names follow quartiq/stabilizer-stream
src/psd.rs so that tests read like the reference's own:

    PsdCascade(n)            PsdCascade::<N>::default()        src/psd.rs:408-423
      .set_detrend(Detrend)  PsdCascade::set_detrend           src/psd.rs:438-443
      .set_avg(AvgOpts)      PsdCascade::set_avg               src/psd.rs:431-436
      .process(x)            PsdCascade::process               src/psd.rs:456-468
      .psd(MergeOpts)        PsdCascade::psd -> (psd, breaks)  src/psd.rs:479-543
    Break.frequencies(b)     Break::frequencies                src/psd.rs:315-327

There is no CPU fallback: constructing a PsdCascade without a HIP device raises.
The directory name carries a hyphen; import it through `__graft_entry__.load_package()`
or tests/conftest.py (module name `stabilizer_stream_amd`).
"""
import ctypes as C
import enum
import importlib.util
import os
import subprocess
import sys
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# $PSDC_LIB: another build of the SAME library (tools/gpu.sh variants: timing-only ablation builds) -- never a fallback
LIB_PATH = os.environ.get("PSDC_LIB") or os.path.join(_HERE, "libpsdcascade.so")
U32_MAX = 0xFFFFFFFF

PSDC_OK = 0
ERR_ARG, ERR_DEVICE, ERR_NOMEM, ERR_UNIMPLEMENTED = -1, -2, -3, -4
ERR_FRAME_HEADER, ERR_FRAME_FORMAT, ERR_FRAME_SIZE, ERR_CAPACITY = -5, -6, -7, -8
OPT_QUANTUM, OPT_PROFILE, OPT_COALESCE, OPT_MIN_PAIRS, OPT_EAGER, OPT_MERGE = 1, 2, 3, 4, 5, 6


class PsdError(RuntimeError):
    """A contract violation the reference would panic on, or a device error."""

    def __init__(self, code, msg):
        super().__init__(f"psdcascade error {code}: {msg}")
        self.code = code


class FrameError(PsdError):
    """de::Error (src/de/mod.rs:19-27)."""


class Detrend(enum.IntEnum):
    """src/psd.rs:59-72"""
    NONE = 0
    MIDPOINT = 1
    SPAN = 2
    MEAN = 3
    LINEAR = 4


class Format(enum.IntEnum):
    """Stream payload formats (src/de/mod.rs:9-17)"""
    ADC_DAC = 1
    FLS = 2
    THERMOSTAT_EEM = 3
    MPLL = 4


# labels of Payload::traces by format (src/de/data.rs:38-80, 98-138, 155, 181-207); trace i feeds channel i (src/bin/psd.rs:174-182)
TRACE_NAMES = {
    Format.ADC_DAC: ("ADC0", "ADC1", "DAC0", "DAC1"),
    Format.FLS: ("AR", "AP", "BI", "BQ"),
    Format.THERMOSTAT_EEM: ("T00", "T20", "I0", "I1"),
    Format.MPLL: ("phase (rad)", "frequency (kHz)", "amplitude (V/G10)"),
}
BATCH_BYTES = {Format.ADC_DAC: 64, Format.FLS: 56, Format.THERMOSTAT_EEM: 80, Format.MPLL: 24}  # src/de/data.rs:13, 86, 144, 168


class Window(enum.IntEnum):
    """Window::rectangular / Window::hann (src/psd.rs:24-55) by kind"""
    RECTANGULAR = 0
    HANN = 1
    CUSTOM = 2


@dataclass(frozen=True, eq=False)
class WindowTable:
    """`Window<N>` (src/psd.rs:12-20): a public struct with public fields, so a caller may build any.

        WindowTable.hann(n) / .rectangular(n)        Window::hann() / Window::rectangular()   src/psd.rs:24-55
        WindowTable(win, power, nenbw, overlap)      Window { win, power, nenbw, overlap }
    """
    win: np.ndarray  # [n] f32
    power: float     # src/psd.rs:15
    nenbw: float     # src/psd.rs:17
    overlap: int     # src/psd.rs:19

    @staticmethod
    def _kind(n, kind):
        w = np.empty(n, dtype=np.float32)
        p, e, ov = C.c_float(), C.c_float(), C.c_size_t()
        rc = lib().psdc_window_table(n, int(kind), _fptr(w), C.byref(p), C.byref(e), C.byref(ov))
        if rc < 0:
            _raise(rc)
        return WindowTable(w, p.value, e.value, ov.value)

    @staticmethod
    def hann(n):
        return WindowTable._kind(n, Window.HANN)

    @staticmethod
    def rectangular(n):
        return WindowTable._kind(n, Window.RECTANGULAR)

    def as_tuple(self):
        """(win, power, nenbw, overlap)"""
        return (self.win, self.power, self.nenbw, self.overlap)


@dataclass(frozen=True)
class MergeOpts:
    """src/psd.rs:339-358"""
    keep_overlap: bool = False
    min_count: int = 1
    keep_transition_band: bool = False


@dataclass(frozen=True)
class AvgOpts:
    """src/psd.rs:360-376"""
    limit: int = U32_MAX
    count: int = U32_MAX


class _CBreak(C.Structure):
    _fields_ = [("start", C.c_uint64), ("include", C.c_uint32), ("count", C.c_uint32),
                ("avg", C.c_uint32), ("_pad", C.c_uint32),
                ("bins_start", C.c_uint64), ("bins_end", C.c_uint64),
                ("fft_size", C.c_uint64), ("decimation", C.c_uint64),
                ("pending", C.c_uint64), ("processed", C.c_uint64)]


class _CStageStat(C.Structure):
    _fields_ = [("count", C.c_uint32), ("avg", C.c_uint32),
                ("pending", C.c_uint64), ("processed", C.c_uint64)]


class _CWfBlocks(C.Structure):
    _fields_ = [("block", C.c_uint32), ("depth", C.c_uint32), ("started", C.c_uint64),
                ("rows_valid", C.c_uint32), ("newest_count", C.c_uint32), ("pending", C.c_uint64)]


class _CLoss(C.Structure):
    _fields_ = [("received", C.c_uint64), ("dropped", C.c_uint64),
                ("next_seq", C.c_uint32), ("have_seq", C.c_uint32)]


class _CProfile(C.Structure):
    _fields_ = [("launches", C.c_uint64), ("kernel_ms", C.c_double),
                ("samples", C.c_uint64), ("stage0_samples", C.c_uint64)]


@dataclass(frozen=True)
class Break:
    """Stage break information (src/psd.rs:290-311)."""
    start: int
    include: bool
    count: int
    avg: int
    bins: range
    fft_size: int
    decimation: int
    pending: int
    processed: int

    def effective_fft_size(self):  # src/psd.rs:329-331
        return self.fft_size * self.decimation

    def rbw(self):  # src/psd.rs:334-336
        return float(np.float32(1.0) / np.float32(self.effective_fft_size()))

    def _c(self):
        return _CBreak(self.start, int(self.include), self.count, self.avg, 0, self.bins.start,
                       self.bins.stop, self.fft_size, self.decimation, self.pending, self.processed)

    @staticmethod
    def _from_c(b):
        return Break(int(b.start), bool(b.include), int(b.count), int(b.avg),
                     range(int(b.bins_start), int(b.bins_end)), int(b.fft_size),
                     int(b.decimation), int(b.pending), int(b.processed))

    @staticmethod
    def frequencies(breaks):
        """Break::frequencies (src/psd.rs:315-327)."""
        L = lib()
        arr = (_CBreak * max(1, len(breaks)))(*[b._c() for b in breaks])
        n = L.psdc_frequencies(arr, len(breaks), None, 0)
        out = np.empty(n, dtype=np.float32)
        L.psdc_frequencies(arr, len(breaks), out.ctypes.data_as(C.POINTER(C.c_float)), n)
        return out


def build(force=False, verbose=False):
    """Compile libpsdcascade.so for gfx950 with hipcc (csrc/Makefile)."""
    csrc = os.path.join(_HERE, "csrc")
    cmd = ["make", "-C", csrc] + (["-B"] if force else [])
    subprocess.run(cmd, check=True, stdout=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def _one_hip_runtime():
    """A process must hold ONE HIP runtime.  PyTorch wheels bundle their own libamdhip64.so; if
    libpsdcascade.so were loaded first it would bind /opt/rocm's copy, torch would later bring its
    own, and whichever initialises second finds "no ROCm-capable device".  So when torch is
    installed but not imported yet, load the runtime it will use (same SONAME) before our library;
    no torch import is forced on callers that never use it."""
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def lib():
    """Load the C-ABI library.  Fails loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run __graft_entry__.build() "
                          "(there is no Python/CPU fallback for the PSD kernels)")
    _one_hip_runtime()
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in _PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _lib = L
    return L


def _prototypes():
    """name -> (restype, argtypes) of every function of include/psdcascade.h.  Built without the library: lib() applies it."""
    P = C.POINTER
    H = vp = C.c_void_p
    u32, u64, i32, sz, fl, text = C.c_uint32, C.c_uint64, C.c_int, C.c_size_t, C.c_float, C.c_char_p
    fp, dp, up, p64, psz, pp = P(fl), P(C.c_double), P(u32), P(u64), P(sz), P(vp)
    stat, brk = P(_CStageStat), P(_CBreak)
    win = [u32, fp, fl, fl, sz]         # n and a window table: the head of every create_window
    opts = [i32, u32, i32]              # MergeOpts
    out = [sz, psz, brk, sz, psz]       # capacity, length written, breaks, their capacity, breaks written
    T = {}

    def f(name, res, args):
        T[name] = (res, args)

    def merged(*rows):
        """a merged read-out of one unit: its rows between the options and the lengths"""
        return [H, u32] + opts + list(rows) + out

    # What every family has.  Per family: the prefix; how many counts create takes between the window and the device; how many
    # sizes supported takes (0: there is no such call); which of set_avg, stats_read and set_carrier it has ("side": the carrier
    # is one of a pair's two); the prefix of its frames pair and loss record.
    for pre, units, sup, has, frames in (
            ("psdc_", 1, 0, "avg", None),   # (its frames calls take no map: they follow)
            ("psdc_cross_", 1, 0, "avg stats", "psdc_csd_"),
            ("psdc_csm_", 2, 2, "avg stats", "psdc_csm_"),
            ("psdc_zoom_", 1, 0, "avg stats carrier", "psdc_zoomcascade_"),
            ("psdc_zcsd_", 1, 1, "avg stats carrier side", "psdc_zoomcsdcascade_"),
            ("psdc_iq_", 1, 0, "avg stats carrier", "psdc_iq_"),
            ("psdc_iqcsd_", 1, 1, "avg stats carrier side", "psdc_iqcsd_"),
            ("psdc_sk_", 1, 1, "avg stats", None),
            ("psdc_zsk_", 1, 1, "avg stats carrier", None),
            ("psdc_iqsk_", 1, 1, "avg stats carrier", None),
            ("psdc_zampm_", 1, 1, "avg stats carrier", None),
            ("psdc_iqampm_", 1, 1, "avg stats carrier", None),
            ("psdc_zxampm_", 1, 1, "avg stats carrier side", None),
            ("psdc_iqxampm_", 1, 1, "avg stats carrier side", None),
            ("psdc_wf_", 3, 1, "stats", None),
            ("psdc_zwf_", 3, 1, "stats carrier", None)):
        has = has.split()
        f(pre + "create", H, [u32, i32] + [u32] * units + [i32])
        f(pre + "create_window", H, win + [u32] * units + [i32])
        f(pre + "destroy", None, [H])
        f(pre + "reset", i32, [H])
        f(pre + "set_detrend", i32, [H, i32])
        f(pre + "sync", i32, [H])
        f(pre + "num_stages", i32, [H, u32])
        f(pre + "last_error", text, [H])
        if sup:
            f(pre + "supported", i32, [u32] * sup)
        if "avg" in has:
            f(pre + "set_avg", i32, [H, u32, u32])
        if "stats" in has:
            f(pre + "stats_read", i32, [H, p64, p64, i32])
        if "carrier" in has:
            f(pre + "set_carrier", i32, [H, u32] + [u32] * ("side" in has) + [u64, u64])
        if frames:
            f(frames + "process_frames", i32, [H, up, vp, sz, sz, psz])
            f(frames + "process_frames_device", i32, [H, up, vp, sz, sz, psz, vp])
            f(frames + "loss_read", i32, [H, P(_CLoss), i32])

    # PsdCascadeBank, Psd and the host helpers
    f("psdc_abi_version", i32, [])
    f("psdc_window_get", i32, [H, P(i32), fp, fp, psz, fp])
    f("psdc_window_table", i32, [u32, i32, fp, fp, fp, psz])
    f("psdc_stitch", i32, [u32, i32, u32, up, up, p64, fp] + opts + [fp] + out)
    f("psdc_stitch_window", i32, [u32, fl, fl, sz, u32, p64, up, p64, fp] + opts + [fp] + out)
    f("psdc_readout_bytes", sz, [u32, u32])
    f("psdc_pack_readout", i32, [H, vp, sz, psz])
    f("psdc_pack_init", i32, [vp, sz, u32, fl, fl, sz, u32])
    f("psdc_pack_channel", i32, [vp, sz, u32, u32, p64, up, p64, fp])
    f("psdc_pack_pad", i32, [vp, sz, vp, sz, u32])
    f("psdc_unpack_info", i32, [vp, sz, u32, up, up, up])
    f("psdc_unpack_stitch", i32, [vp, sz, u32] + opts + [fp] + out)
    f("psdc_clone", H, [H])
    f("psdc_configure", i32, [H, i32, C.c_int64])
    f("psdc_process", i32, [H, u32, fp, sz])
    f("psdc_process_device", i32, [H, u32, vp, sz])
    f("psdc_process_device_after", i32, [H, u32, vp, sz, vp])
    f("psdc_record_consumed", i32, [H, vp])
    for name in ("psdc_process_adcdac_frames", "psdc_process_frames", "psdc_process_frames_device",
                 "psdc_process_adcdac_frames_device"):
        f(name, i32, [H, vp, sz, sz, psz])
    f("psdc_loss_read", i32, [H, P(_CLoss), i32])
    f("psdc_flush", i32, [H])
    f("psdc_stage_info", i32, [H, u32, u32, stat])
    f("psdc_stage_spectrum", i32, [H, u32, u32, fp])
    f("psdc_stage_gain", i32, [H, u32, u32, fp])
    f("psdc_stage_buf", i32, [H, u32, u32, fp, sz, psz])
    f("psdc_read_channel", i32, [H, u32, u32, up, stat, fp])
    f("psdc_psd", i32, merged(fp))
    f("psdc_rbw", fl, [H])
    f("psdc_frequencies", sz, [brk, sz, fp, sz])
    f("psdc_hbf_response_length", i32, [i32])
    f("psdc_plan_counts", i32, [u32, i32, u64, u32, p64, p64, p64])
    f("psdc_var_eval", fl, [i32, i32, fl, sz, fp, fp, sz, fl])
    f("psdc_hbf_dec8", i32, [i32, fp, sz, fp])
    f("psdc_fill_noise_device", i32, [i32, vp, sz, u64, u64])
    f("psdc_profile_read", i32, [H, P(_CProfile), i32])
    f("psdc_trace_plot", i32, [fp, fp, sz, fl, i32, fl, fl, fp, dp, sz, psz])
    f("psdc_stage_create", H, [u32, i32, i32])
    f("psdc_stage_create_window", H, win + [i32])
    f("psdc_stage_destroy", None, [H])
    f("psdc_stage_clone", H, [H])
    f("psdc_stage_set_avg", i32, [H, u32])
    f("psdc_stage_set_detrend", i32, [H, i32])
    f("psdc_stage_process", i32, [H, fp, sz, fp, sz, psz])
    f("psdc_stage_process_device", i32, [H, vp, sz, vp, sz, psz])
    f("psdc_stage_get_spectrum", i32, [H, fp])
    f("psdc_stage_get_count", i32, [H, up])
    f("psdc_stage_get_gain", i32, [H, fp])
    f("psdc_stage_get_buf", i32, [H, fp, sz, psz])
    f("psdc_stage_last_error", text, [H])

    # The feeds.  f32 streams: one real stream a unit, two (a pair), planar I and Q, interleaved (re, im); _device forms take
    # device addresses and, last, an event to wait for.
    for pre in ("psdc_zoom_", "psdc_sk_", "psdc_zsk_", "psdc_zampm_", "psdc_wf_", "psdc_zwf_"):
        f(pre + "process", i32, [H, u32, fp, sz])
        f(pre + "process_device", i32, [H, u32, vp, sz, vp])
    for pre in ("psdc_cross_", "psdc_zcsd_", "psdc_zxampm_"):
        f(pre + "process", i32, [H, u32, fp, fp, sz])
        f(pre + "process_device", i32, [H, u32, vp, vp, sz, vp])
    for pre in ("psdc_iq_", "psdc_iqsk_", "psdc_iqampm_"):
        f(pre + "process", i32, [H, u32, fp, fp, sz])
        f(pre + "process_device", i32, [H, u32, vp, vp, sz, vp])
        f(pre + "process_interleaved", i32, [H, u32, fp, sz])
        f(pre + "process_interleaved_device", i32, [H, u32, vp, sz, vp])
    for pre in ("psdc_iqcsd_", "psdc_iqxampm_"):
        f(pre + "process", i32, [H, u32, fp, fp, fp, fp, sz])
        f(pre + "process_device", i32, [H, u32, vp, vp, vp, vp, sz, vp])
        f(pre + "process_interleaved", i32, [H, u32, fp, fp, sz])
        f(pre + "process_interleaved_device", i32, [H, u32, vp, vp, sz, vp])
    f("psdc_csm_process", i32, [H, u32, pp, sz])
    f("psdc_csm_process_device", i32, [H, u32, pp, sz, vp])
    # integer streams (kind, scale): one stream a unit, two, or m behind a pointer table
    for pre in ("psdc_sint_", "psdc_int_zoom_", "psdc_int_iq_"):
        f(pre + "process", i32, [H, u32, vp, i32, fl, sz])
        f(pre + "process_device", i32, [H, u32, vp, i32, fl, sz, vp])
    for pre in ("psdc_sint_cross_", "psdc_int_zcsd_", "psdc_int_iqcsd_"):
        f(pre + "process", i32, [H, u32, vp, vp, i32, fl, sz])
        f(pre + "process_device", i32, [H, u32, vp, vp, i32, fl, sz, vp])
    f("psdc_sint_csm_process", i32, [H, u32, pp, i32, fl, sz])
    f("psdc_sint_csm_process_device", i32, [H, u32, pp, i32, fl, sz, vp])

    # stage reads and read-outs, family by family
    f("psdc_cross_stage_spectra", i32, [H, u32, u32, stat, fp, fp, fp])
    f("psdc_cross_csd", i32, merged(fp, fp, fp))
    f("psdc_cross_stitch", i32, [u32, fl, fl, sz, u32, p64, up, p64, fp] + opts + [fp, fp, fp] + out)
    f("psdc_csm_stage_spectra", i32, [H, u32, u32, stat, fp])
    f("psdc_csm_csd", i32, merged(fp))
    f("psdc_csm_stitch", i32, [u32, u32, fl, fl, sz, u32, p64, up, p64, fp] + opts + [fp] + out)
    for pre in ("psdc_zoom_", "psdc_iq_"):
        f(pre + "stage_spectra", i32, [H, u32, u32, stat, fp, fp])
        f(pre + "psd", i32, merged(fp, fp))
    for pre in ("psdc_zcsd_", "psdc_iqcsd_"):
        f(pre + "stage_spectra", i32, [H, u32, u32, stat, fp])
        f(pre + "csd", i32, merged(*[fp] * 6))
    f("psdc_sk_stage_moments", i32, [H, u32, u32, stat, dp, dp])
    f("psdc_sk_psd", i32, merged(fp))
    f("psdc_sk_sk", i32, merged(dp))
    for pre in ("psdc_zsk_", "psdc_iqsk_"):
        f(pre + "stage_moments", i32, [H, u32, u32, stat, dp, dp, dp, dp])
        f(pre + "psd", i32, merged(fp, fp))
        f(pre + "sk", i32, merged(dp, dp))
    for pre in ("psdc_zampm_", "psdc_iqampm_"):
        f(pre + "stage_rows", i32, [H, u32, u32, stat, dp, dp, dp, dp])
        f(pre + "psd", i32, merged(fp, fp))
        f(pre + "sidebands", i32, merged(dp, dp, dp, dp))
    for pre in ("psdc_zxampm_", "psdc_iqxampm_"):
        f(pre + "stage_rows", i32, [H, u32, u32, stat, dp])
        f(pre + "sidebands", i32, merged(dp))
    for pre, nrows in (("psdc_wf_", 2), ("psdc_zwf_", 4)):
        f(pre + "stage_blocks", i32, [H, u32, u32, P(_CWfBlocks)])
        f(pre + "stage_rows", i32, [H, u32, u32, u32, p64, up] + [dp] * nrows + [up])
        f(pre + "image", i32, [H, u32, u32, u32, fp, fp, p64, up, up])
        f(pre + "image_device", i32, [H, u32, u32, u32, vp, vp, p64, up, up])
    return T


_PROTOTYPES = _prototypes()
EXPORTS = list(_PROTOTYPES)


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class SampleKind(enum.IntEnum):
    """The integer sample kinds of the psdc_int_* calls (PSDC_SAMPLE_*).  For the complex objects a unit is an interleaved
    (re, im) pair of the kind's integers: sc16, sc8."""
    S16 = 1
    S8 = 2


def sample_kind(dtype):
    """(SampleKind, default scale) of an integer dtype: int16 -> (S16, 2^-15), int8 -> (S8, 2^-7), so full scale maps into
    [-1, 1).  The one place that maps a dtype to a kind; any other dtype raises ValueError."""
    dt = np.dtype(dtype)
    if dt == np.dtype(np.int16):
        return SampleKind.S16, 2.0 ** -15
    if dt == np.dtype(np.int8):
        return SampleKind.S8, 2.0 ** -7
    raise ValueError(f"integer samples are int16 or int8, not {dt}")


def int_samples(x):
    """(array, kind, default scale) of a real integer stream for process_int: a 1-D C-contiguous int16 or int8 array, taken as
    it is (never converted or copied); anything else raises ValueError."""
    if not isinstance(x, np.ndarray):
        raise ValueError("integer samples are a numpy array of int16 or int8")
    kind, scale = sample_kind(x.dtype)
    if x.ndim != 1:
        raise ValueError(f"a real integer stream is 1-D, not of shape {x.shape}")
    if not x.flags.c_contiguous:
        raise ValueError("the integer samples are not contiguous")
    return x, kind, scale


def int_pairs(z):
    """(array, kind, default scale) of a complex integer stream for process_int: a C-contiguous int16 or int8 array of shape
    (len, 2) holding (re, im) rows (sc16, sc8), taken as it is; anything else raises ValueError."""
    if not isinstance(z, np.ndarray):
        raise ValueError("integer samples are a numpy array of int16 or int8")
    kind, scale = sample_kind(z.dtype)
    if z.ndim != 2 or z.shape[1] != 2:
        raise ValueError(f"a complex integer stream has the shape (len, 2), not {z.shape}")
    if not z.flags.c_contiguous:
        raise ValueError("the (re, im) integer pairs are not contiguous")
    return z, kind, scale


def _int_scale(kind, scale):
    """the kind as the C ABI takes it and the scale (None: the kind's default)"""
    if scale is None:
        kind = SampleKind(kind)
        scale = 2.0 ** -15 if kind == SampleKind.S16 else 2.0 ** -7
    return int(kind), float(scale)


def _same_kind(a, b):
    if a[0].dtype != b[0].dtype or a[0].shape != b[0].shape:
        raise ValueError(f"the two sides differ in dtype or shape ({a[0].dtype} {a[0].shape} and {b[0].dtype} {b[0].shape})")


def _raise(code, h=None):
    msg = lib().psdc_last_error(h)
    msg = msg.decode() if msg else ""
    cls = FrameError if code in (ERR_FRAME_HEADER, ERR_FRAME_FORMAT, ERR_FRAME_SIZE) else PsdError
    raise cls(code, msg)


def _stage_info(st):
    """a _CStageStat as the info dict of the stage reads"""
    return {"count": st.count, "avg": st.avg, "pending": st.pending, "processed": st.processed}


def _carrier_words(f0, ftw, phase0):
    """(ftw, phase0) modulo 2^64 of a carrier given as exactly one of f0 (through zoom_ftw) and ftw"""
    if (f0 is None) == (ftw is None):
        raise PsdError(ERR_ARG, "give exactly one of f0 and ftw")
    if ftw is None:
        ftw = zoom_ftw(f0)[0]
    return int(ftw) % (1 << 64), int(phase0) % (1 << 64)


class _Bank:
    """What the banks share: one handle `_h` of the C ABI, made by the create or create_window of the family whose C prefix is
    `_P`, that family's error text, and the calls every family has.  A bank class sets the attributes below, mixes in what its
    family has beside them (_SetAvg, _Stats, _FramesFeed, a carrier mixin) and keeps its own feeds, stage reads and read-outs."""

    _P = None                                                        # the family's C prefix, e.g. "psdc_zoom_"
    _ARG_WORDS = ("must be", "out of range", "null", "window_kind")  # a failed create is ERR_ARG if its message has one
    _IN = "samples_in"                                               # the second key of stats_read

    def _open(self, n, window, device, *units):
        """The handle, by create or, for a WindowTable, create_window; `units` are the family's counts between the window and
        the device (channels, pairs, ...), which the frames map builder takes too."""
        self.n, self.window, self.device, self._units = n, window, device, units
        self._L = lib()
        if isinstance(window, WindowTable):
            w = np.ascontiguousarray(window.win, dtype=np.float32)
            if w.size != n:
                raise PsdError(ERR_ARG, "window table length != n")
            self._h = self._f("create_window")(n, _fptr(w), window.power, window.nenbw, window.overlap, *units, device)
        else:
            self._h = self._f("create")(n, int(window), *units, device)
        if not self._h:
            self._create_failed()
        self._fresh(65536)

    def _create_failed(self):
        msg = self._f("last_error")(None)
        msg = msg.decode() if msg else ""
        raise PsdError(ERR_ARG if any(w in msg for w in self._ARG_WORDS) else ERR_DEVICE, msg)

    def _fresh(self, most=None):
        """What the binding keeps beside the handle (carriers, detrend), as create and reset leave it; `most` caps a table."""

    def _f(self, name):
        return getattr(self._L, self._P + name)

    def close(self):
        if getattr(self, "_h", None):
            self._f("destroy")(self._h)
            self._h = None

    __del__ = close

    def _ck(self, rc):
        if rc < 0:
            msg = self._f("last_error")(self._h)
            cls = FrameError if rc in (ERR_FRAME_HEADER, ERR_FRAME_FORMAT, ERR_FRAME_SIZE) else PsdError
            raise cls(rc, msg.decode() if msg else "")
        return rc

    def reset(self):
        """Back to a fresh object: what the binding keeps beside the handle (the carriers: ftw = 0, phase0 = 0) too."""
        self._ck(self._f("reset")(self._h))
        self._fresh()

    def set_detrend(self, d):
        self._ck(self._f("set_detrend")(self._h, int(d)))

    def sync(self):
        self._ck(self._f("sync")(self._h))

    def _num_stages(self, unit):
        return self._ck(self._f("num_stages")(self._h, unit))

    def _merged(self, fn, unit, opts, widths, dtype=np.float32):
        """One merged read-out call `fn` of `unit`.  widths: per row the numbers it holds a bin (1, or 2 for a complex row of
        (re, im)), each row behind a pointer of its own; or an int: that many rows of one number a bin as one [rows][capacity]
        array behind one pointer.  Returns (the rows cut to the bins written, in memory of their own, the breaks)."""
        ns = self._num_stages(unit)
        cap = max(1, ns * (self.n // 2 + 1))
        cp = C.POINTER(C.c_double if dtype == np.float64 else C.c_float)
        if isinstance(widths, int):
            rows = np.zeros((widths, cap), dtype)
            ptrs = [rows.ctypes.data_as(cp)]
        else:
            rows = [np.empty(w * cap, dtype) for w in widths]
            ptrs = [r.ctypes.data_as(cp) for r in rows]
        br = (_CBreak * max(1, ns))()
        plen, nb = C.c_size_t(), C.c_size_t()
        self._ck(fn(self._h, unit, int(opts.keep_overlap), opts.min_count, int(opts.keep_transition_band), *ptrs, cap,
                    C.byref(plen), br, ns, C.byref(nb)))
        m = plen.value
        rows = rows[:, :m] if isinstance(widths, int) else [r[:w * m].copy() for r, w in zip(rows, widths)]
        return rows, [Break._from_c(br[i]) for i in range(nb.value)]

    def _process_iq(self, channel, z):
        """The complex-stream process of the family: z a complex array (process_interleaved) or a pair (i, q) (process)."""
        if isinstance(z, (tuple, list)):
            if len(z) != 2:
                raise PsdError(ERR_ARG, "a planar call takes (i, q)")
            i = np.ascontiguousarray(z[0], dtype=np.float32)
            q = np.ascontiguousarray(z[1], dtype=np.float32)
            if i.ndim != 1 or i.shape != q.shape:
                raise PsdError(ERR_ARG, f"i and q differ in length ({i.size} and {q.size})")
            self._ck(self._f("process")(self._h, channel, _fptr(i), _fptr(q), i.size))
            return
        z = np.asarray(z)
        if not np.iscomplexobj(z):
            raise PsdError(ERR_ARG, "process takes a complex array or a pair (i, q)")
        z = np.ascontiguousarray(z, dtype=np.complex64)
        self._ck(self._f("process_interleaved")(self._h, channel, _fptr(z), z.size))

    def _process_iq_pair(self, pair, za, zb):
        """_process_iq for a pair: two complex arrays, or two pairs (ia, qa), (ib, qb)."""
        planar = [isinstance(z, (tuple, list)) for z in (za, zb)]
        if all(planar):
            if len(za) != 2 or len(zb) != 2:
                raise PsdError(ERR_ARG, "a planar call takes (ia, qa), (ib, qb)")
            x = [np.ascontiguousarray(v, dtype=np.float32) for v in (*za, *zb)]
            if any(v.ndim != 1 or v.shape != x[0].shape for v in x):
                raise PsdError(ERR_ARG, "the four streams differ in length (" + ", ".join(str(v.size) for v in x) + ")")
            self._ck(self._f("process")(self._h, pair, *[_fptr(v) for v in x], x[0].size))
            return
        if any(planar):
            raise PsdError(ERR_ARG, "process takes two complex arrays or two pairs (i, q), not one of each")
        za, zb = np.asarray(za), np.asarray(zb)
        if not (np.iscomplexobj(za) and np.iscomplexobj(zb)):
            raise PsdError(ERR_ARG, "process takes two complex arrays or two pairs (i, q)")
        za = np.ascontiguousarray(za, dtype=np.complex64)
        zb = np.ascontiguousarray(zb, dtype=np.complex64)
        if za.ndim != 1 or za.shape != zb.shape:
            raise PsdError(ERR_ARG, f"za and zb differ in length ({za.size} and {zb.size})")
        self._ck(self._f("process_interleaved")(self._h, pair, _fptr(za), _fptr(zb), za.size))


class _SetAvg:
    """set_avg, for every family but the waterfalls"""

    def set_avg(self, avg):
        self._ck(self._f("set_avg")(self._h, avg.limit, avg.count))


class _Stats:
    """stats_read, for every family but PsdCascadeBank (which has profile_read); `_IN` names what the family counts"""

    def stats_read(self, reset=False):
        la, si = C.c_uint64(), C.c_uint64()
        self._ck(self._f("stats_read")(self._h, C.byref(la), C.byref(si), int(reset)))
        return {"launches": la.value, self._IN: si.value}


class _ChannelBank(_SetAvg, _Stats, _Bank):
    """A bank of `n_channels` units fed one stream each."""

    def __init__(self, n, n_channels=1, window=Window.HANN, device=0):
        self.n_channels = n_channels
        self._open(n, window, device, n_channels)

    def num_stages(self, channel=0):
        return self._num_stages(channel)


class _PairBank(_SetAvg, _Stats, _Bank):
    """A bank of `n_pairs` units fed two streams each."""

    _IN = "pairs_in"

    def __init__(self, n, n_pairs=1, window=Window.HANN, device=0):
        self.n_pairs = n_pairs
        self._open(n, window, device, n_pairs)

    def num_stages(self, pair=0):
        return self._num_stages(pair)


class _FramesFeed:
    """The stream-frames feed of a bank.  `_FP` is the C prefix of its process_frames pair and loss record (not always the
    family's own), `_MAP` the builder of the trace map: called with what the caller names and the bank's unit counts."""

    _FP = None
    _MAP = None

    def _frames(self, data, frame_size, entries):
        buf = np.frombuffer(data, dtype=np.uint8)
        m = self._MAP(entries, *self._units)
        ok = C.c_size_t(0)
        self._ck(getattr(self._L, self._FP + "process_frames")(
            self._h, m.ctypes.data_as(C.POINTER(C.c_uint32)), buf.ctypes.data_as(C.c_void_p), frame_size,
            buf.size // frame_size, C.byref(ok)))
        return ok.value

    def _frames_device(self, ptr, frame_size, n_frames, entries, after):
        m = self._MAP(entries, *self._units)
        ok = C.c_size_t(0)
        self._ck(getattr(self._L, self._FP + "process_frames_device")(
            self._h, m.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_void_p(ptr), frame_size, n_frames, C.byref(ok),
            C.c_void_p(after) if after else None))
        return ok.value

    def loss(self, reset=False):
        """Loss counters (src/loss.rs) over the frames ingested: batches received / dropped."""
        l = _CLoss()
        self._ck(getattr(self._L, self._FP + "loss_read")(self._h, C.byref(l), int(reset)))
        return {"received": l.received, "dropped": l.dropped}


class _ChannelCarriers:
    """A carrier per channel: `carriers[c]` is the (ftw, phase0) of channel c, as set."""

    def _fresh(self, most=None):
        super()._fresh(most)
        self.carriers = {c: (0, 0) for c in range(self.n_channels if most is None else min(self.n_channels, most))}

    def set_carrier(self, channel, f0=None, ftw=None, phase0=0):
        """The channel's carrier, as f0 (cycles per sample, through zoom_ftw) or as the tuning word itself; phase0 in 2^-64
        turn.  Only before the channel's first sample.  Returns the f0 actually used."""
        ftw, phase0 = _carrier_words(f0, ftw, phase0)
        self._ck(self._f("set_carrier")(self._h, channel, ftw, phase0))
        self.carriers[channel] = (ftw, phase0)
        return ftw / float(1 << 64)


class _SideCarriers:
    """A carrier per side of a pair: the table named by `_CARRIERS` holds the (ftw, phase0) of (pair, side), as set."""

    _CARRIERS = "carriers"
    _SIDES = "0: channel a, 1: channel b"

    def _fresh(self, most=None):
        super()._fresh(most)
        if most is None:
            keys = getattr(self, self._CARRIERS)
        else:
            keys = [(p, s) for p in range(min(self.n_pairs, most)) for s in (0, 1)]
        setattr(self, self._CARRIERS, {k: (0, 0) for k in keys})

    def set_carrier(self, pair, f0=None, ftw=None, phase0=0, side=None):
        """The carrier of one side of a pair (side 0: a, 1: b) or, with side=None, of both; as f0 (cycles per sample, through
        zoom_ftw) or as the tuning word itself; phase0 in 2^-64 turn.  Only before the pair's first sample.  Returns the f0
        actually used."""
        ftw, phase0 = _carrier_words(f0, ftw, phase0)
        if side is not None and side not in (0, 1):
            raise PsdError(ERR_ARG, f"side {side} out of range ({self._SIDES})")
        for s in ((0, 1) if side is None else (side,)):
            self._ck(self._f("set_carrier")(self._h, pair, s, ftw, phase0))
            getattr(self, self._CARRIERS)[(pair, s)] = (ftw, phase0)
        return ftw / float(1 << 64)


class PsdCascadeBank(_FramesFeed, _SetAvg, _Bank):
    """`n_channels` independent PsdCascade<N> batched on one GPU (one handle of the C ABI)."""

    _P = _FP = "psdc_"

    def __init__(self, n, n_channels=1, window=Window.HANN, device=0, _handle=None):
        """window: a Window kind, or a caller-built WindowTable (any Window<N>, src/psd.rs:12-20).
        device: HIP device index, or -1 = the index in $PSDC_DEVICE (0 when unset)."""
        self.n_channels = n_channels
        if _handle is None:
            self._open(n, window, device, n_channels)
        else:
            self.n, self.window, self.device, self._L, self._h = n, window, device, lib(), _handle

    def _create_failed(self):
        _raise(ERR_DEVICE)

    def window_get(self):
        """(kind, WindowTable) as the library holds it: a table equal to Window::hann() is recognised as HANN."""
        k, p, e, ov = C.c_int(), C.c_float(), C.c_float(), C.c_size_t()
        w = np.empty(self.n, dtype=np.float32)
        self._ck(self._L.psdc_window_get(self._h, C.byref(k), C.byref(p), C.byref(e), C.byref(ov), _fptr(w)))
        return Window(k.value), WindowTable(w, p.value, e.value, ov.value)

    def pack_readout(self):
        """psdc_pack_readout: the fixed-size byte record of this handle's raw accumulators and counters."""
        need = self._L.psdc_readout_bytes(self.n, self.n_channels)
        buf = np.empty(need, dtype=np.uint8)
        ln = C.c_size_t()
        self._ck(self._L.psdc_pack_readout(self._h, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(ln)))
        assert ln.value == need
        return buf

    def clone(self):
        h = self._L.psdc_clone(self._h)
        if not h:
            _raise(ERR_DEVICE)
        return PsdCascadeBank(self.n, self.n_channels, self.window, self.device, _handle=h)

    def configure(self, quantum=None, profile=None, coalesce=None, min_pairs=None, eager=None, merge=None):
        if merge is not None:
            self._ck(self._L.psdc_configure(self._h, OPT_MERGE, int(bool(merge))))
        if eager is not None:
            self._ck(self._L.psdc_configure(self._h, OPT_EAGER, int(bool(eager))))
        if min_pairs is not None:
            self._ck(self._L.psdc_configure(self._h, OPT_MIN_PAIRS, int(min_pairs)))
        if quantum is not None:
            self._ck(self._L.psdc_configure(self._h, OPT_QUANTUM, int(quantum)))
        if profile is not None:
            self._ck(self._L.psdc_configure(self._h, OPT_PROFILE, int(bool(profile))))
        if coalesce is not None:
            self._ck(self._L.psdc_configure(self._h, OPT_COALESCE, int(coalesce)))

    def rbw(self):
        return float(self._L.psdc_rbw(self._h))

    def process(self, channel, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        self._ck(self._L.psdc_process(self._h, channel, _fptr(x), x.size))

    def process_device(self, channel, ptr, length, after=None):
        """ptr: device address (e.g. torch tensor .data_ptr()) of `length` f32 samples.  The producer of the
        samples must have completed -- or pass `after`: a hipEvent_t handle (torch.cuda.Event.cuda_event)
        recorded behind the producing work; the library's stream then waits for it on the device."""
        if after is None:
            self._ck(self._L.psdc_process_device(self._h, channel, C.c_void_p(ptr), length))
        else:
            self._ck(self._L.psdc_process_device_after(self._h, channel, C.c_void_p(ptr), length, C.c_void_p(after)))

    def process_int(self, channel, x, scale=None):
        """x: a 1-D C-contiguous int16 or int8 array, fed as it is (psdc_sint_process): the library sees float32(v) *
        float32(scale), scale None = the dtype's default (2^-15, 2^-7: full scale into [-1, 1)).  The same staging, quantum and
        fast path as process; one (kind, scale) in the same call sizes gives the bits of process fed the converted stream."""
        x, kind, dflt = int_samples(x)
        self._ck(self._L.psdc_sint_process(self._h, channel, x.ctypes.data_as(C.c_void_p), int(kind),
                                           dflt if scale is None else float(scale), x.size))

    def process_int_device(self, channel, ptr, length, kind, scale=None, after=None):
        """ptr: device address of `length` integers of SampleKind `kind`; after as process_device.  The integers are converted
        into the stage-0 stream buffer (one extra pass: they are not read in place as a long f32 span is); they must stay
        unchanged until sync(), a read-out or a record_consumed event."""
        kind, scale = _int_scale(kind, scale)
        self._ck(self._L.psdc_sint_process_device(self._h, channel, C.c_void_p(ptr), kind, scale, length,
                                                  C.c_void_p(after) if after else None))

    def record_consumed(self, event):
        """Record the hipEvent_t handle `event` behind the last read of every span handed over so far."""
        self._ck(self._L.psdc_record_consumed(self._h, C.c_void_p(event)))

    def _ingest(self, fn, ptr, frame_size, n_frames):
        ok = C.c_size_t(0)
        self._ck(fn(self._h, ptr, frame_size, n_frames, C.byref(ok)))
        return ok.value

    def process_adcdac_frames(self, data, frame_size):
        """data: bytes-like holding whole frames; returns the number of frames ingested."""
        buf = np.frombuffer(data, dtype=np.uint8)
        return self._ingest(self._L.psdc_process_adcdac_frames, buf.ctypes.data_as(C.c_void_p), frame_size, buf.size // frame_size)

    def process_frames(self, data, frame_size):
        """Frames of any of the four payload formats (src/de/mod.rs:12-17), each frame's own header naming its format: trace i of
        every frame goes to channel i.  data: bytes-like holding whole frames; returns the number of frames ingested."""
        buf = np.frombuffer(data, dtype=np.uint8)
        return self._ingest(self._L.psdc_process_frames, buf.ctypes.data_as(C.c_void_p), frame_size, buf.size // frame_size)

    def process_frames_device(self, ptr, frame_size, n_frames):
        """process_frames for frames resident in device memory at address `ptr`; returns the number of frames ingested."""
        return self._ingest(self._L.psdc_process_frames_device, C.c_void_p(ptr), frame_size, n_frames)

    def process_adcdac_frames_device(self, ptr, frame_size, n_frames):
        """Frames resident in device memory at address `ptr`; returns the number of frames ingested."""
        return self._ingest(self._L.psdc_process_adcdac_frames_device, C.c_void_p(ptr), frame_size, n_frames)

    def flush(self):
        self._ck(self._L.psdc_flush(self._h))

    def num_stages(self, channel=0):
        return self._num_stages(channel)

    def stage_info(self, channel, stage):
        st = _CStageStat()
        self._ck(self._L.psdc_stage_info(self._h, channel, stage, C.byref(st)))
        return _stage_info(st)

    def stage_spectrum(self, channel, stage):
        out = np.empty(self.n // 2 + 1, dtype=np.float32)
        self._ck(self._L.psdc_stage_spectrum(self._h, channel, stage, _fptr(out)))
        return out

    def stage_gain(self, channel, stage):
        g = C.c_float()
        self._ck(self._L.psdc_stage_gain(self._h, channel, stage, C.byref(g)))
        return g.value

    def stage_buf(self, channel, stage):
        ln = C.c_size_t()
        self._ck(self._L.psdc_stage_buf(self._h, channel, stage, None, 0, C.byref(ln)))
        out = np.empty(ln.value, dtype=np.float32)
        self._ck(self._L.psdc_stage_buf(self._h, channel, stage, _fptr(out), out.size, C.byref(ln)))
        return out

    def read_channel(self, channel=0):
        """All stages of one channel in one call: ([{count, avg, pending, processed}], spectra[ns, n/2+1])."""
        ns = C.c_uint32()
        self._ck(self._L.psdc_read_channel(self._h, channel, 0, C.byref(ns), None, None))
        st = (_CStageStat * max(1, ns.value))()
        sp = np.empty((ns.value, self.n // 2 + 1), dtype=np.float32)
        self._ck(self._L.psdc_read_channel(self._h, channel, ns.value, C.byref(ns), st, _fptr(sp) if ns.value else None))
        return [_stage_info(st[k]) for k in range(ns.value)], sp

    def psd(self, channel=0, opts=MergeOpts()):
        (p,), br = self._merged(self._L.psdc_psd, channel, opts, (1,))
        return p, br

    def profile_read(self, reset=False):
        p = _CProfile()
        self._ck(self._L.psdc_profile_read(self._h, C.byref(p), int(reset)))
        return {"launches": p.launches, "kernel_ms": p.kernel_ms, "samples": p.samples,
                "stage0_samples": p.stage0_samples}


class _Cascade:
    """What the single objects share: a bank `_b` of the class `_BANK` with one unit, and the calls that name no unit."""

    _BANK = None

    def __init__(self, n, window=Window.HANN, device=0):
        self.n = n
        self._b = self._BANK(n, 1, window, device)

    def set_detrend(self, d):
        self._b.set_detrend(d)

    def num_stages(self):
        return self._b.num_stages(0)

    def sync(self):
        self._b.sync()

    def close(self):
        self._b.close()


class _UnitCascade(_Cascade):
    """The single object of every bank but PsdCascadeBank and the waterfalls: set_avg, reset and stats_read beside the above."""

    def set_avg(self, avg):
        self._b.set_avg(avg)

    def reset(self):
        self._b.reset()

    def stats_read(self, reset=False):
        return self._b.stats_read(reset)


class _KeepsCarrier:
    """A single object around one carrier, over a bank with _ChannelCarriers: `f0` is the frequency in use (ftw / 2^64), and
    reset() keeps the carrier."""

    def _tune(self, f0, ftw, phase0):
        if f0 is None and ftw is None:
            ftw = 0
        self.set_carrier(f0=f0, ftw=ftw, phase0=phase0)

    def set_carrier(self, f0=None, ftw=None, phase0=0):
        self.f0 = self._b.set_carrier(0, f0=f0, ftw=ftw, phase0=phase0)
        self.ftw, self.phase0 = self._b.carriers[0]
        return self.f0

    def reset(self):
        self._b.reset()
        self._b.set_carrier(0, ftw=self.ftw, phase0=self.phase0)


class _CarrierCascade(_KeepsCarrier, _UnitCascade):
    """One stream around one carrier: the single object of the zoom and IQ banks."""

    def __init__(self, n, f0=None, ftw=None, phase0=0, window=Window.HANN, device=0):
        super().__init__(n, window, device)
        self._tune(f0, ftw, phase0)

    def process(self, x):
        self._b.process(0, x)

    def process_device(self, ptr, length, after=None):
        self._b.process_device(0, ptr, length, after)

    def psd(self, opts=MergeOpts()):
        return self._b.psd(0, opts)


class _PairCarrierCascade(_UnitCascade):
    """One pair around a carrier a side, over a bank with _SideCarriers: the constructor's carrier goes to both sides, and
    reset() keeps both."""

    def __init__(self, n, f0=None, ftw=None, phase0=0, window=Window.HANN, device=0):
        super().__init__(n, window, device)
        if f0 is None and ftw is None:
            ftw = 0
        self.set_carrier(f0=f0, ftw=ftw, phase0=phase0)

    def set_carrier(self, f0=None, ftw=None, phase0=0, side=None):
        f = self._b.set_carrier(0, f0=f0, ftw=ftw, phase0=phase0, side=side)
        table = getattr(self._b, self._BANK._CARRIERS)
        setattr(self, self._BANK._CARRIERS, [table[(0, 0)], table[(0, 1)]])
        return f

    def process(self, x, y):
        self._b.process(0, x, y)

    def process_device(self, px, py, length, after=None):
        self._b.process_device(0, px, py, length, after)

    def csd(self, opts=MergeOpts()):
        return self._b.csd(0, opts)

    def reset(self):
        car = list(getattr(self, self._BANK._CARRIERS))
        self._b.reset()
        for s, (ftw, ph) in enumerate(car):
            self._b.set_carrier(0, ftw=ftw, phase0=ph, side=s)


class PsdCascade(_Cascade):
    """Online cascaded PSD estimator, one trace (src/psd.rs:399-544)."""

    def __init__(self, n, window=Window.HANN, device=0, _bank=None):
        self.n = n
        self._b = _bank if _bank is not None else PsdCascadeBank(n, 1, window, device)

    def clone(self):
        return PsdCascade(self.n, _bank=self._b.clone())

    def rbw(self):
        return self._b.rbw()

    def set_avg(self, avg):
        self._b.set_avg(avg)

    def process(self, x):
        self._b.process(0, x)

    def process_device(self, ptr, length, after=None):
        self._b.process_device(0, ptr, length, after)

    def process_int(self, x, scale=None):
        self._b.process_int(0, x, scale)

    def process_int_device(self, ptr, length, kind, scale=None, after=None):
        self._b.process_int_device(0, ptr, length, kind, scale, after)

    def psd(self, opts=MergeOpts()):
        return self._b.psd(0, opts)

    # PsdStage accessors of stage i (src/psd.rs:271-287)
    def stage_spectrum(self, i):
        return self._b.stage_spectrum(0, i)

    def stage_gain(self, i):
        return self._b.stage_gain(0, i)

    def stage_count(self, i):
        return self._b.stage_info(0, i)["count"]

    def stage_buf(self, i):
        return self._b.stage_buf(0, i)

    def stage_info(self, i):
        return self._b.stage_info(0, i)

    def configure(self, **kw):
        self._b.configure(**kw)


TRACE_NONE = 0xFFFFFFFF


def trace_index(t):
    """A trace of Payload::traces as its index: an int, or a TRACE_NAMES label (the labels of the four formats are distinct)."""
    if isinstance(t, str):
        for names in TRACE_NAMES.values():
            if t in names:
                return names.index(t)
        raise PsdError(ERR_ARG, f"unknown trace label {t!r}")
    return int(t)


def pair_map(pairs, n_pairs):
    """The psdc_csd_* map of `pairs`: entry p is (x, y) -- trace indices or TRACE_NAMES labels -- or None (pair p not fed);
    pairs past the end of the list are not fed."""
    if len(pairs) > n_pairs:
        raise PsdError(ERR_ARG, f"{len(pairs)} pairs for a bank of {n_pairs}")
    m = np.full(2 * n_pairs, TRACE_NONE, np.uint32)
    for p, xy in enumerate(pairs):
        if xy is not None:
            m[2 * p], m[2 * p + 1] = trace_index(xy[0]), trace_index(xy[1])
    return m


class CsdCascadeBank(_FramesFeed, _PairBank):
    """`n_pairs` independent cross-spectral cascades (psdc_cross_*): pairs of streams x, y fed together.  Per stage the
    accumulators Sxx, Syy and Sxy = sum conj(X) Y (scipy.signal.csd's convention: H1 = Sxy / Sxx); the read-out is
    PsdCascade::psd (src/psd.rs:479-543) applied to each row, so Sxx is the psd() of a PsdCascade fed x."""

    _P, _FP, _MAP = "psdc_cross_", "psdc_csd_", staticmethod(pair_map)

    def process(self, pair, x, y):
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.ascontiguousarray(y, dtype=np.float32)
        if x.size != y.size:
            raise PsdError(ERR_ARG, "x and y must have equal lengths")
        self._ck(self._L.psdc_cross_process(self._h, pair, _fptr(x), _fptr(y), x.size))

    def process_device(self, pair, px, py, length, after=None):
        """px, py: device addresses of `length` f32 samples each; after: a hipEvent_t handle recorded behind their
        producer (torch.cuda.Event.cuda_event), or None when the producer has completed.  The samples must stay
        unchanged until sync() or a read-out returns."""
        self._ck(self._L.psdc_cross_process_device(self._h, pair, C.c_void_p(px), C.c_void_p(py), length,
                                                   C.c_void_p(after) if after else None))

    def process_int(self, pair, x, y, scale=None):
        """x, y: 1-D int16 or int8 arrays of one dtype and length, fed as they are (psdc_sint_cross_process): the bits of
        process fed float32(v) * float32(scale); scale None = the dtype's default"""
        a, b = int_samples(x), int_samples(y)
        _same_kind(a, b)
        self._ck(self._L.psdc_sint_cross_process(self._h, pair, a[0].ctypes.data_as(C.c_void_p), b[0].ctypes.data_as(C.c_void_p),
                                                 int(a[1]), a[2] if scale is None else float(scale), a[0].size))

    def process_int_device(self, pair, px, py, length, kind, scale=None, after=None):
        """px, py: device addresses of `length` integers of SampleKind `kind` each; the rest as process_device"""
        kind, scale = _int_scale(kind, scale)
        self._ck(self._L.psdc_sint_cross_process_device(self._h, pair, C.c_void_p(px), C.c_void_p(py), kind, scale, length,
                                                        C.c_void_p(after) if after else None))

    def process_frames(self, data, frame_size, pairs):
        """Stream frames of any of the four payload formats (bytes-like holding whole frames) into the pairs: pairs[p] = (x, y)
        feeds pair p with traces x and y of every frame (indices or TRACE_NAMES labels), None leaves it unfed.  Returns the
        number of frames ingested; a bad frame raises FrameError after the frames before it were ingested."""
        return self._frames(data, frame_size, pairs)

    def process_frames_device(self, ptr, frame_size, n_frames, pairs, after=None):
        """process_frames for frames resident in device memory at address `ptr`; after: a hipEvent_t handle recorded behind
        their producer, or None when it has completed.  The payloads must stay unchanged until sync() or a read-out returns."""
        return self._frames_device(ptr, frame_size, n_frames, pairs, after)

    def stage_spectra(self, pair, stage):
        """(info, sxx, syy, sxy) of one stage's raw accumulators; sxy complex64."""
        b = self.n // 2 + 1
        st = _CStageStat()
        xx, yy, xy = np.empty(b, np.float32), np.empty(b, np.float32), np.empty(2 * b, np.float32)
        self._ck(self._L.psdc_cross_stage_spectra(self._h, pair, stage, C.byref(st), _fptr(xx), _fptr(yy), _fptr(xy)))
        return _stage_info(st), xx, yy, xy.view(np.complex64)

    def csd(self, pair=0, opts=MergeOpts()):
        """(sxx, syy, sxy complex64, breaks): PsdCascade::psd of each row."""
        (xx, yy, xy), br = self._merged(self._L.psdc_cross_csd, pair, opts, (1, 1, 2))
        return xx, yy, xy.view(np.complex64), br


class CsdCascade(_UnitCascade):
    """One pair of streams: the cross-spectral form of PsdCascade (src/psd.rs:393 names `csdl` as its model)."""

    _BANK = CsdCascadeBank

    def process(self, x, y):
        self._b.process(0, x, y)

    def process_device(self, px, py, length, after=None):
        self._b.process_device(0, px, py, length, after)

    def process_int(self, x, y, scale=None):
        self._b.process_int(0, x, y, scale)

    def process_int_device(self, px, py, length, kind, scale=None, after=None):
        self._b.process_int_device(0, px, py, length, kind, scale, after)

    def process_frames(self, data, frame_size, pair):
        """pair: (x, y) traces of the frames (CsdCascadeBank.process_frames)"""
        return self._b.process_frames(data, frame_size, [pair])

    def process_frames_device(self, ptr, frame_size, n_frames, pair, after=None):
        return self._b.process_frames_device(ptr, frame_size, n_frames, [pair], after)

    def loss(self, reset=False):
        return self._b.loss(reset)

    def csd(self, opts=MergeOpts()):
        return self._b.csd(0, opts)

    def stage_spectra(self, i):
        return self._b.stage_spectra(0, i)


def group_map(groups, m, n_groups):
    """The psdc_csm_* map of `groups`: entry g is m traces -- indices or TRACE_NAMES labels -- or None (group g not fed);
    groups past the end of the list are not fed."""
    if len(groups) > n_groups:
        raise PsdError(ERR_ARG, f"{len(groups)} groups for a bank of {n_groups}")
    out = np.full(m * n_groups, TRACE_NONE, np.uint32)
    for g, tr in enumerate(groups):
        if tr is None:
            continue
        if len(tr) != m:
            raise PsdError(ERR_ARG, f"group {g} names {len(tr)} traces for m = {m}")
        out[m * g:m * g + m] = [trace_index(t) for t in tr]
    return out


def csm_supported(n, m):
    """Whether CsmCascadeBank(n, m) can be created (psdc_csm_supported; pure host code)."""
    return bool(0 <= n < 2 ** 32 and 0 <= m < 2 ** 32 and lib().psdc_csm_supported(n, m))


def csm_matrix(rows, m):
    """The Hermitian matrix (m, m, bins) complex64 of m*m real rows in the layout of include/psdcascade.h: row a*m + a is
    S_aa, for a < b row a*m + b is Re S_ab and row b*m + a is Im S_ab.  Both sides filled, S[b, a] = conj(S[a, b])."""
    rows = np.asarray(rows, np.float32).reshape(m * m, -1)
    S = np.zeros((m, m, rows.shape[1]), np.complex64)
    for a in range(m):
        S[a, a] = rows[a * m + a]
        for b in range(a + 1, m):
            S[a, b].real, S[a, b].imag = rows[a * m + b], rows[b * m + a]
            S[b, a] = np.conj(S[a, b])
    return S


class CsmCascadeBank(_FramesFeed, _SetAvg, _Stats, _Bank):
    """`n_groups` independent cross-spectral MATRIX cascades (psdc_csm_*): groups of m = 2 ... 4 streams fed together, each
    transformed and decimated once a segment; per stage the Hermitian matrix S_ab = sum conj(X_a) X_b (the pair object's
    convention).  The read-out is PsdCascade::psd applied to each real row: S[a, a] is the psd() of a PsdCascade fed channel a."""

    _P, _FP, _MAP = "psdc_csm_", "psdc_csm_", staticmethod(group_map)
    _ARG_WORDS = _Bank._ARG_WORDS + ("not supported",)
    _IN = "sample_times_in"

    def __init__(self, n, m, n_groups=1, window=Window.HANN, device=0):
        self.m, self.n_groups = m, n_groups
        if not (0 <= n < 2 ** 32 and 0 <= m < 2 ** 32):
            raise PsdError(ERR_ARG, f"n = {n} with m = {m} is not supported")
        self._open(n, window, device, m, n_groups)

    def _ptrs(self, ptrs):
        if len(ptrs) != self.m:
            raise PsdError(ERR_ARG, f"{len(ptrs)} channels for m = {self.m}")
        return (C.c_void_p * self.m)(*ptrs)

    def process(self, group, xs):
        """xs: m arrays of equal length, one per channel of the group"""
        xs = [np.ascontiguousarray(x, dtype=np.float32) for x in xs]
        if len({x.size for x in xs}) > 1:
            raise PsdError(ERR_ARG, "the channels of a group must have equal lengths")
        arr = self._ptrs([x.ctypes.data for x in xs])
        self._ck(self._L.psdc_csm_process(self._h, group, arr, xs[0].size))

    def process_device(self, group, ptrs, length, after=None):
        """ptrs: m device addresses of `length` f32 samples each; after: a hipEvent_t handle recorded behind their producer
        (torch.cuda.Event.cuda_event), or None when the producer has completed.  The samples must stay unchanged until
        sync() or a read-out returns."""
        self._ck(self._L.psdc_csm_process_device(self._h, group, self._ptrs([int(p) for p in ptrs]), length,
                                                 C.c_void_p(after) if after else None))

    def process_int(self, group, xs, scale=None):
        """xs: m 1-D int16 or int8 arrays of one dtype and length, fed as they are (psdc_sint_csm_process): the bits of process
        fed float32(v) * float32(scale); scale None = the dtype's default"""
        if isinstance(xs, np.ndarray) or len(xs) != self.m:
            raise ValueError(f"a group takes a list of m = {self.m} integer arrays")
        a = [int_samples(x) for x in xs]
        for b in a[1:]:
            _same_kind(a[0], b)
        arr = (C.c_void_p * self.m)(*[x[0].ctypes.data for x in a])
        self._ck(self._L.psdc_sint_csm_process(self._h, group, arr, int(a[0][1]), a[0][2] if scale is None else float(scale),
                                               a[0][0].size))

    def process_int_device(self, group, ptrs, length, kind, scale=None, after=None):
        """ptrs: m device addresses of `length` integers of SampleKind `kind` each; the rest as process_device"""
        if len(ptrs) != self.m:
            raise ValueError(f"{len(ptrs)} channels for m = {self.m}")
        kind, scale = _int_scale(kind, scale)
        self._ck(self._L.psdc_sint_csm_process_device(self._h, group, (C.c_void_p * self.m)(*[int(p) for p in ptrs]), kind, scale,
                                                      length, C.c_void_p(after) if after else None))

    def process_frames(self, data, frame_size, groups):
        """Stream frames (bytes-like holding whole frames) into the groups: groups[g] = m traces (indices or TRACE_NAMES
        labels) feeds group g, None leaves it unfed.  Returns the number of frames ingested; a bad frame raises FrameError
        after the frames before it were ingested."""
        return self._frames(data, frame_size, groups)

    def process_frames_device(self, ptr, frame_size, n_frames, groups, after=None):
        """process_frames for frames resident in device memory at address `ptr` (CsdCascadeBank.process_frames_device)."""
        return self._frames_device(ptr, frame_size, n_frames, groups, after)

    def num_stages(self, group=0):
        return self._num_stages(group)

    def stage_spectra(self, group, stage):
        """(info, S) of one stage's raw accumulators; S complex64 (m, m, n/2 + 1), Hermitian."""
        st = _CStageStat()
        rows = np.empty(self.m * self.m * (self.n // 2 + 1), np.float32)
        self._ck(self._L.psdc_csm_stage_spectra(self._h, group, stage, C.byref(st), _fptr(rows)))
        return _stage_info(st), csm_matrix(rows, self.m)

    def csd(self, group=0, opts=MergeOpts()):
        """(S, breaks): S complex64 (m, m, bins), Hermitian and filled on both sides; PsdCascade::psd of each real row."""
        rows, br = self._merged(self._L.psdc_csm_csd, group, opts, self.m * self.m)
        return csm_matrix(rows, self.m), br


class CsmCascade(_UnitCascade):
    """One group of m streams (CsmCascadeBank with n_groups = 1)."""

    def __init__(self, n, m, window=Window.HANN, device=0):
        self.n, self.m = n, m
        self._b = CsmCascadeBank(n, m, 1, window, device)

    def process(self, xs):
        self._b.process(0, xs)

    def process_device(self, ptrs, length, after=None):
        self._b.process_device(0, ptrs, length, after)

    def process_int(self, xs, scale=None):
        self._b.process_int(0, xs, scale)

    def process_int_device(self, ptrs, length, kind, scale=None, after=None):
        self._b.process_int_device(0, ptrs, length, kind, scale, after)

    def process_frames(self, data, frame_size, group):
        return self._b.process_frames(data, frame_size, [group])

    def process_frames_device(self, ptr, frame_size, n_frames, group, after=None):
        return self._b.process_frames_device(ptr, frame_size, n_frames, [group], after)

    def loss(self, reset=False):
        return self._b.loss(reset)

    def csd(self, opts=MergeOpts()):
        return self._b.csd(0, opts)

    def stage_spectra(self, i):
        return self._b.stage_spectra(0, i)


def zoom_ftw(f0):
    """(ftw, f0 used): the 64-bit frequency tuning word of a carrier at f0 cycles per sample, round(f0 2^64) mod 2^64, and the
    frequency ftw / 2^64 it stands for.  f0 may be a float, a Fraction or anything Fraction() takes: the product is exact."""
    from fractions import Fraction
    ftw = round(Fraction(f0) * (1 << 64)) % (1 << 64)
    return ftw, ftw / float(1 << 64)


def two_sided(upper, lower, breaks):
    """(offsets, density) of a zoom read-out as one two-sided spectrum: the offsets from the carrier in cycles per sample,
    ascending from -0.5 to 0.5, with the density at each: `lower` mirrored, then `upper`.  Offset 0 (in both rows) appears once,
    from `upper`; so does Nyquist, at +0.5."""
    f = np.asarray(Break.frequencies(breaks), np.float64)
    up, lo = np.asarray(upper), np.asarray(lower)
    order = np.argsort(f, kind="stable")
    f, up, lo = f[order], up[order], lo[order]
    neg = (f > 0) & (f < 0.5)
    return np.concatenate([-f[neg][::-1], f]), np.concatenate([lo[neg][::-1], up])


def channel_map(traces, n_channels):
    """The map psdc_zoomcascade_process_frames[_device] take, from `traces`: entry c is the trace channel c takes -- an index or a TRACE_NAMES label (trace_index, as
    pair_map resolves its pairs) -- or None (channel c not fed); channels past the end of the list are not fed.  A map that
    feeds no channel, an index outside 0 ... 3 and an unknown label are ERR_ARG here, before the library sees the call."""
    traces = list(traces)
    if len(traces) > n_channels:
        raise PsdError(ERR_ARG, f"{len(traces)} traces for a bank of {n_channels}")
    m = np.full(n_channels, TRACE_NONE, np.uint32)
    for c, t in enumerate(traces):
        if t is None:
            continue
        i = trace_index(t)
        if not 0 <= i < 4:
            raise PsdError(ERR_ARG, f"channel {c} names trace {i} (frames carry at most 4)")
        m[c] = i
    if not np.any(m != TRACE_NONE):
        raise PsdError(ERR_ARG, "the map feeds no channel")
    return m


class ZoomCascadeBank(_ChannelCarriers, _FramesFeed, _ChannelBank):
    """`n_channels` independent zoom cascades (psdc_zoom_*): each real stream is mixed down from its own carrier (a 64-bit
    tuning word and start phase, exact in integers) to I + i Q in front of the cascade, and every stage keeps the two-sided
    |Z|^2 of it as two rows: `upper` at offset f is the PSD of x at f0 + f, `lower` that at f0 - f, both scaled as
    PsdCascade::psd scales its one-sided spectrum (white noise of variance 1 reads 2)."""

    _P, _FP, _MAP = "psdc_zoom_", "psdc_zoomcascade_", staticmethod(channel_map)

    def process(self, channel, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        self._ck(self._L.psdc_zoom_process(self._h, channel, _fptr(x), x.size))

    def process_device(self, channel, ptr, length, after=None):
        """ptr: device address of `length` f32 samples; after: a hipEvent_t handle recorded behind their producer, or None
        when it has completed.  The samples must stay unchanged until sync() or a read-out returns."""
        self._ck(self._L.psdc_zoom_process_device(self._h, channel, C.c_void_p(ptr), length,
                                                  C.c_void_p(after) if after else None))

    def process_int(self, channel, x, scale=None):
        """x: a 1-D int16 or int8 array, fed as it is; the mixer sees float32(v) * float32(scale) (scale None: 2^-15 for int16,
        2^-7 for int8) and gives the bits process() gives for that stream."""
        x, kind, dflt = int_samples(x)
        self._ck(self._L.psdc_int_zoom_process(self._h, channel, x.ctypes.data_as(C.c_void_p), int(kind),
                                               dflt if scale is None else float(scale), x.size))

    def process_int_device(self, channel, ptr, length, kind, scale=None, after=None):
        """ptr: device address of `length` integers of SampleKind `kind`, aligned to the integer; the rest as process_device"""
        kind, scale = _int_scale(kind, scale)
        self._ck(self._L.psdc_int_zoom_process_device(self._h, channel, C.c_void_p(ptr), kind, scale, length,
                                                      C.c_void_p(after) if after else None))

    def process_frames(self, data, frame_size, traces):
        """Stream frames of any of the four payload formats (bytes-like holding whole frames) into the channels: traces[c] is the
        trace channel c takes of every frame (an index or a TRACE_NAMES label), None leaves it unfed; a trace may feed several
        channels.  The frames are decoded and mixed on the device in one kernel.  Returns the number of frames ingested; a bad
        frame raises FrameError after the frames before it were ingested."""
        return self._frames(data, frame_size, traces)

    def process_frames_device(self, ptr, frame_size, n_frames, traces, after=None):
        """process_frames for frames resident in device memory at address `ptr`; after: a hipEvent_t handle recorded behind
        their producer, or None when it has completed.  The payloads must stay unchanged until sync() or a read-out returns."""
        return self._frames_device(ptr, frame_size, n_frames, traces, after)

    def stage_spectra(self, channel, stage):
        """(info, upper, lower) of one stage's raw accumulators."""
        b = self.n // 2 + 1
        st = _CStageStat()
        up, lo = np.empty(b, np.float32), np.empty(b, np.float32)
        self._ck(self._f("stage_spectra")(self._h, channel, stage, C.byref(st), _fptr(up), _fptr(lo)))
        return _stage_info(st), up, lo

    def psd(self, channel=0, opts=MergeOpts()):
        """(upper, lower, breaks): PsdCascade::psd of each row; Break.frequencies(breaks) are the offsets of both, and
        two_sided(upper, lower, breaks) is the spectrum over (-0.5, 0.5]."""
        (up, lo), br = self._merged(self._f("psd"), channel, opts, (1, 1))
        return up, lo, br


class ZoomCascade(_CarrierCascade):
    """One stream around one carrier: ZoomCascade(n, f0=0.2) or ZoomCascade(n, ftw=...).  `f0` is the frequency in use
    (ftw / 2^64).  reset() keeps the object's carrier."""

    _BANK = ZoomCascadeBank

    def process_int(self, x, scale=None):
        self._b.process_int(0, x, scale)

    def process_int_device(self, ptr, length, kind, scale=None, after=None):
        self._b.process_int_device(0, ptr, length, kind, scale, after)

    def process_frames(self, data, frame_size, trace):
        """trace: the trace of the frames the stream is (ZoomCascadeBank.process_frames)"""
        return self._b.process_frames(data, frame_size, [trace])

    def process_frames_device(self, ptr, frame_size, n_frames, trace, after=None):
        return self._b.process_frames_device(ptr, frame_size, n_frames, [trace], after)

    def loss(self, reset=False):
        return self._b.loss(reset)

    def stage_spectra(self, i):
        return self._b.stage_spectra(0, i)


def sk_supported(n):
    """Whether SkCascade[Bank] takes the size n: a power of two 64 ... 4096"""
    return 0 <= n < (1 << 32) and bool(lib().psdc_sk_supported(n))


def sk_from_moments(count, s1, s2):
    """The spectral kurtosis estimator over M = count averaged segments, in f64, from the moments S1 = sum P and S2 = sum P^2
    of the periodogram:  SK = (M + 1) / (M - 1) * (M S2 / S1^2 - 1).  1 for Gaussian noise of any colour (2 at the real-valued
    bins 0 and N/2), 0 for a line of constant amplitude, about 2/d - 1 for noise present a fraction d of the time.  NaN for
    count < 2 and where S1 == 0."""
    s1, s2 = np.asarray(s1, np.float64), np.asarray(s2, np.float64)
    m = float(count)
    if count < 2:
        return np.full(np.broadcast(s1, s2).shape, np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        sk = (m + 1.0) / (m - 1.0) * (m * s2 / (s1 * s1) - 1.0)
    return np.where(s1 == 0.0, np.nan, sk)


def sk_sigma(count):
    """2 / sqrt(count): the asymptotic standard deviation of a bin of sk_from_moments for Gaussian noise over `count` independent
    segments.  It ignores the small correlation of 50 %-overlapped Hann segments (which widens the scatter slightly) and is
    not meant below a few tens of averages."""
    return 2.0 / float(np.sqrt(float(count)))


class SkCascadeBank(_ChannelBank):
    """`n_channels` independent spectral kurtosis cascades (psdc_sk_*): every stage of a real stream keeps S1 = sum P, the
    spectrum PsdCascade keeps, and S2 = sum P^2 beside it.  psd() is PsdCascade's; sk() is the per-bin estimator
    sk_from_moments of the same stages and bins: 1 where the bin holds stationary Gaussian noise."""

    _P = "psdc_sk_"

    def process(self, channel, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        self._ck(self._L.psdc_sk_process(self._h, channel, _fptr(x), x.size))

    def process_device(self, channel, ptr, length, after=None):
        """ptr: device address of `length` f32 samples; after: a hipEvent_t handle recorded behind their producer, or None
        when it has completed.  The samples must stay unchanged until sync() or a read-out returns."""
        self._ck(self._L.psdc_sk_process_device(self._h, channel, C.c_void_p(ptr), length, C.c_void_p(after) if after else None))

    def stage_moments(self, channel, stage):
        """(info, s1, s2) of one stage: its raw f64 accumulators sum w P and sum w P^2"""
        b = self.n // 2 + 1
        st = _CStageStat()
        s1, s2 = np.empty(b, np.float64), np.empty(b, np.float64)
        dp = C.POINTER(C.c_double)
        self._ck(self._L.psdc_sk_stage_moments(self._h, channel, stage, C.byref(st), s1.ctypes.data_as(dp), s2.ctypes.data_as(dp)))
        return _stage_info(st), s1, s2

    def psd(self, channel=0, opts=MergeOpts()):
        """(psd, breaks): PsdCascade::psd of row 0, as PsdCascade.psd() returns it"""
        (p,), br = self._merged(self._L.psdc_sk_psd, channel, opts, (1,))
        return p, br

    def sk(self, channel=0, opts=MergeOpts()):
        """(sk, breaks): float64 SK of every bin of psd(), from the stage and bin psd() took it from; the same breaks"""
        (s,), br = self._merged(self._L.psdc_sk_sk, channel, opts, (1,), np.float64)
        return s, br

    stats = _Stats.stats_read


class SkCascade(_UnitCascade):
    """One stream: SkCascade(n).  psd() beside sk(), the per-bin spectral kurtosis."""

    _BANK = SkCascadeBank

    def process(self, x):
        self._b.process(0, x)

    def process_device(self, ptr, length, after=None):
        self._b.process_device(0, ptr, length, after)

    def psd(self, opts=MergeOpts()):
        return self._b.psd(0, opts)

    def sk(self, opts=MergeOpts()):
        return self._b.sk(0, opts)

    def stage_moments(self, i):
        return self._b.stage_moments(0, i)

    stats = _UnitCascade.stats_read


def iq_map(pairs, n_channels):
    """The map psdc_iq_process_frames[_device] take, from `pairs`: entry c is the (i_trace, q_trace) channel c takes -- indices or
    TRACE_NAMES labels (trace_index, as channel_map resolves its traces), e.g. ("BI", "BQ") -- or None (channel c not fed);
    channels past the end of the list are not fed.  A map that feeds no channel, a pair with one None, an index outside 0 ... 3
    and an unknown label are ERR_ARG here, before the library sees the call."""
    pairs = list(pairs)
    if len(pairs) > n_channels:
        raise PsdError(ERR_ARG, f"{len(pairs)} trace pairs for a bank of {n_channels}")
    m = np.full(2 * n_channels, TRACE_NONE, np.uint32)
    for c, pq in enumerate(pairs):
        if pq is None:
            continue
        if not isinstance(pq, (tuple, list)) or len(pq) != 2 or pq[0] is None or pq[1] is None:
            raise PsdError(ERR_ARG, f"channel {c} needs a pair (i_trace, q_trace)")
        for side, t in enumerate(pq):
            i = trace_index(t)
            if not 0 <= i < 4:
                raise PsdError(ERR_ARG, f"channel {c} names trace {i} (frames carry at most 4)")
            m[2 * c + side] = i
    if not np.any(m != TRACE_NONE):
        raise PsdError(ERR_ARG, "the map feeds no channel")
    return m


class IqCascadeBank(ZoomCascadeBank):
    """`n_channels` independent IQ cascades (psdc_iq_*): each stream is complex already, z = I + i Q, and is turned by its own
    carrier (default none: ftw = 0, phase0 = 0) in front of the zoom object's cascade.  Every stage keeps the two-sided |Z|^2 as
    two rows, `upper` at offsets f >= 0 and `lower` at -f, scaled as PsdCascade::psd scales its one-sided spectrum: complex
    white noise with E|z|^2 = 1 reads 2, and row / 2 is the two-sided density of z (two_sided() lays the rows out)."""

    _P, _FP, _MAP = "psdc_iq_", "psdc_iq_", staticmethod(iq_map)

    def process(self, channel, z):
        """z: a complex array (converted to complex64 and fed as (re, im) pairs: the interleaved route), or a pair (i, q) of
        real arrays of one length (the planar route)."""
        self._process_iq(channel, z)

    def process_device(self, channel, ptr, length, after=None):
        """ptr: device address of `length` (re, im) pairs of f32 (a complex64 tensor's memory; 8-byte aligned); after: a hipEvent_t
        handle recorded behind their producer, or None when it has completed.  The samples must stay unchanged until sync() or a
        read-out returns."""
        self._ck(self._L.psdc_iq_process_interleaved_device(self._h, channel, C.c_void_p(ptr), length,
                                                            C.c_void_p(after) if after else None))

    def process_int(self, channel, z, scale=None):
        """z: a C-contiguous int16 or int8 array of shape (len, 2), the (re, im) rows of sc16 / sc8, fed as it is; the mixer sees
        float32(v) * float32(scale) (scale None: 2^-15 for int16, 2^-7 for int8) and gives the bits process() gives for that
        complex64 stream."""
        z, kind, dflt = int_pairs(z)
        self._ck(self._L.psdc_int_iq_process(self._h, channel, z.ctypes.data_as(C.c_void_p), int(kind),
                                             dflt if scale is None else float(scale), z.shape[0]))

    def process_int_device(self, channel, ptr, length, kind, scale=None, after=None):
        """ptr: device address of `length` (re, im) integer pairs of SampleKind `kind`, aligned to the pair; the rest as
        process_device"""
        kind, scale = _int_scale(kind, scale)
        self._ck(self._L.psdc_int_iq_process_device(self._h, channel, C.c_void_p(ptr), kind, scale, length,
                                                    C.c_void_p(after) if after else None))

    def process_device_planar(self, channel, pi, pq, length, after=None):
        """pi, pq: device addresses of `length` f32 samples each, the I and the Q stream (process_device's rules)"""
        self._ck(self._L.psdc_iq_process_device(self._h, channel, C.c_void_p(pi), C.c_void_p(pq), length,
                                                C.c_void_p(after) if after else None))

    def process_frames(self, data, frame_size, pairs):
        """Stream frames of any of the four payload formats (bytes-like holding whole frames) into the channels: pairs[c] is the
        (i_trace, q_trace) channel c takes of every frame (indices or TRACE_NAMES labels, e.g. ("BI", "BQ")), None leaves it
        unfed; a trace may feed several channels.  The frames are decoded and mixed on the device in one kernel.  Returns the
        number of frames ingested; a bad frame raises FrameError after the frames before it were ingested."""
        return self._frames(data, frame_size, pairs)

    def process_frames_device(self, ptr, frame_size, n_frames, pairs, after=None):
        """process_frames for frames resident in device memory at address `ptr`; after: a hipEvent_t handle recorded behind
        their producer, or None when it has completed.  The payloads must stay unchanged until sync() or a read-out returns."""
        return self._frames_device(ptr, frame_size, n_frames, pairs, after)


class IqCascade(ZoomCascade):
    """One complex stream: IqCascade(n) analyses it as it is, IqCascade(n, f0=0.2) or IqCascade(n, ftw=...) retunes it first.
    `f0` is the frequency in use (ftw / 2^64).  reset() keeps the object's carrier."""

    _BANK = IqCascadeBank

    def process(self, z):
        """z: a complex array, or a pair (i, q) (IqCascadeBank.process)"""
        self._b.process(0, z)

    def process_int(self, z, scale=None):
        self._b.process_int(0, z, scale)

    def process_device_planar(self, pi, pq, length, after=None):
        self._b.process_device_planar(0, pi, pq, length, after)

    def process_frames(self, data, frame_size, pair):
        """pair: the (i_trace, q_trace) of the frames the stream is (IqCascadeBank.process_frames)"""
        return self._b.process_frames(data, frame_size, [pair])

    def process_frames_device(self, ptr, frame_size, n_frames, pair, after=None):
        return self._b.process_frames_device(ptr, frame_size, n_frames, [pair], after)


def zoom_sk_supported(n):
    """Whether ZoomSkCascade[Bank] and IqSkCascade[Bank] take the size n: a power of two 64 ... 4096 (sk_supported)"""
    return 0 <= n < (1 << 32) and bool(lib().psdc_zsk_supported(n))


class ZoomSkCascadeBank(_ChannelCarriers, _ChannelBank):
    """`n_channels` independent zoom spectral kurtosis cascades (psdc_zsk_*): ZoomCascadeBank's carrier, mixer and two-sided
    cascade, with S2 = sum |Z|^4 kept beside S1 = sum |Z|^2 on both sides.  psd() is ZoomCascadeBank's; sk() is sk_from_moments
    of the same stages and bins, per side: 1 where the sideband holds stationary (circular) Gaussian noise, at every bin --
    offset 0 and Nyquist included, every bin of a complex stream being complex; 0 on a line; about 2/d - 1 for power that is on
    a fraction d of the time.  A real stream is not circular where its own DC and Nyquist fall (offset f0 in `lower`,
    0.5 - f0 in `upper`): there SK rises towards 2.  two_sided() lays either read-out out over (-0.5, 0.5]."""

    _P = "psdc_zsk_"

    def process(self, channel, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        self._ck(self._L.psdc_zsk_process(self._h, channel, _fptr(x), x.size))

    def process_device(self, channel, ptr, length, after=None):
        """ptr: device address of `length` f32 samples; after: a hipEvent_t handle recorded behind their producer, or None
        when it has completed.  The samples must stay unchanged until sync() or a read-out returns."""
        self._ck(self._L.psdc_zsk_process_device(self._h, channel, C.c_void_p(ptr), length, C.c_void_p(after) if after else None))

    def stage_moments(self, channel, stage):
        """(info, s1_upper, s1_lower, s2_upper, s2_lower) of one stage: its raw f64 accumulators sum w |Z|^2 and sum w |Z|^4"""
        b = self.n // 2 + 1
        st = _CStageStat()
        rows = [np.empty(b, np.float64) for _ in range(4)]
        dp = C.POINTER(C.c_double)
        self._ck(self._f("stage_moments")(self._h, channel, stage, C.byref(st), *(r.ctypes.data_as(dp) for r in rows)))
        return (_stage_info(st), *rows)

    def psd(self, channel=0, opts=MergeOpts()):
        """(upper, lower, breaks): the zoom read-out of the S1 rows, as ZoomCascadeBank.psd() returns it"""
        rows, br = self._merged(self._f("psd"), channel, opts, (1, 1))
        return (*rows, br)

    def sk(self, channel=0, opts=MergeOpts()):
        """(sk_upper, sk_lower, breaks): float64 SK of every bin of psd(), from the stage and bin psd() took it from"""
        rows, br = self._merged(self._f("sk"), channel, opts, (1, 1), np.float64)
        return (*rows, br)

    stats = _Stats.stats_read


class IqSkCascadeBank(ZoomSkCascadeBank):
    """`n_channels` independent IQ spectral kurtosis cascades (psdc_iqsk_*): ZoomSkCascadeBank for streams that are complex
    already, fed as IqCascadeBank is and turned by an optional carrier (default none).  Circular complex Gaussian noise reads 1
    at every bin of both sides."""

    _P = "psdc_iqsk_"

    def process(self, channel, z):
        """z: a complex array (converted to complex64 and fed as (re, im) pairs: the interleaved route), or a pair (i, q) of
        real arrays of one length (the planar route)."""
        self._process_iq(channel, z)

    def process_device(self, channel, ptr, length, after=None):
        """ptr: device address of `length` (re, im) pairs of f32 (a complex64 tensor's memory; 8-byte aligned); the rest as
        ZoomSkCascadeBank.process_device"""
        self._ck(self._L.psdc_iqsk_process_interleaved_device(self._h, channel, C.c_void_p(ptr), length,
                                                              C.c_void_p(after) if after else None))

    def process_device_planar(self, channel, pi, pq, length, after=None):
        """pi, pq: device addresses of `length` f32 samples each, the I and the Q stream (process_device's rules)"""
        self._ck(self._L.psdc_iqsk_process_device(self._h, channel, C.c_void_p(pi), C.c_void_p(pq), length,
                                                  C.c_void_p(after) if after else None))


class ZoomSkCascade(_CarrierCascade):
    """One real stream around one carrier: ZoomSkCascade(n, f0=0.2) or ZoomSkCascade(n, ftw=...): psd() beside sk(), both
    two-sided.  `f0` is the frequency in use (ftw / 2^64).  reset() keeps the object's carrier."""

    _BANK = ZoomSkCascadeBank
    stats = _UnitCascade.stats_read

    def sk(self, opts=MergeOpts()):
        return self._b.sk(0, opts)

    def stage_moments(self, i):
        return self._b.stage_moments(0, i)


class IqSkCascade(ZoomSkCascade):
    """One complex stream: IqSkCascade(n) analyses it as it is, IqSkCascade(n, f0=0.2) or IqSkCascade(n, ftw=...) retunes it
    first.  process() takes a complex array or a pair (i, q), as IqCascade.process does."""

    _BANK = IqSkCascadeBank

    def process_device_planar(self, pi, pq, length, after=None):
        self._b.process_device_planar(0, pi, pq, length, after)


def waterfall_supported(n):
    """Whether WaterfallCascade[Bank] takes the size n (sk_supported)"""
    return 0 <= n < (1 << 32) and bool(lib().psdc_wf_supported(n))


def zoom_waterfall_supported(n):
    """Whether ZoomWaterfallCascade[Bank] takes the size n (zoom_sk_supported)"""
    return 0 <= n < (1 << 32) and bool(lib().psdc_zwf_supported(n))


def waterfall_block_span(n, overlap, block, stage, b):
    """range of the input samples that block b of `stage` of a waterfall cascade nominally covers:
    [b B hop 8^stage, ((b + 1) B - 1) hop 8^stage + n 8^stage) with hop = n - overlap.  The decimators' delay is not included: a
    deeper stage's blocks lie later in input time by it."""
    hop, d = n - overlap, 8 ** stage
    return range(b * block * hop * d, ((b + 1) * block - 1) * hop * d + n * d)


class WaterfallCascadeBank(_Stats, _Bank):
    """`n_channels` independent waterfall cascades (psdc_wf_*): SkCascadeBank's stages, but every stage keeps a ring of its
    `depth` most recent blocks of `block` segments, each with its own S1 = sum P and S2 = sum P^2, where SkCascadeBank keeps one
    average.  image() gives a stage's PSD and spectral kurtosis against time, oldest block first; stage k's blocks are 8^k times
    longer than stage 0's.  Every segment has weight 1: there is no set_avg."""

    _P = "psdc_wf_"
    _ROWS = 2

    def __init__(self, n, n_channels=1, block=64, depth=64, window=Window.HANN, device=0):
        self.n_channels, self.block, self.depth = n_channels, block, depth
        bad = [k for k, v in (("n", n), ("n_channels", n_channels), ("block", block), ("depth", depth)) if not 0 <= v <= U32_MAX]
        if bad:
            raise PsdError(ERR_ARG, f"{self._P}create: {bad[0]} must be in [0, 2^32)")
        self._open(n, window, device, n_channels, block, depth)
        self._wt = window if isinstance(window, WindowTable) else None

    def _table(self):
        if self._wt is None:
            self._wt = WindowTable._kind(self.n, self.window)
        return self._wt

    def process(self, channel, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        self._ck(self._f("process")(self._h, channel, _fptr(x), x.size))

    def process_device(self, channel, ptr, length, after=None):
        """ptr: device address of `length` f32 samples; after: a hipEvent_t handle recorded behind their producer, or None
        when it has completed.  The samples must stay unchanged until sync() or a read-out returns."""
        self._ck(self._f("process_device")(self._h, channel, C.c_void_p(ptr), length, C.c_void_p(after) if after else None))

    def num_stages(self, channel=0):
        return self._num_stages(channel)

    def stage_blocks(self, channel, stage):
        """dict(block, depth, started, rows_valid, newest_count, pending) of one stage's ring"""
        b = _CWfBlocks()
        self._ck(self._f("stage_blocks")(self._h, channel, stage, C.byref(b)))
        return {k: int(getattr(b, k)) for k, _ in _CWfBlocks._fields_}

    def _cap(self, max_rows):
        cap = self.depth if max_rows is None else int(max_rows)
        if not 0 <= cap <= U32_MAX:
            raise PsdError(ERR_ARG, "max_rows must be in [0, 2^32)")
        return min(cap, self.depth)

    def stage_rows(self, channel, stage, max_rows=None):
        """(block_index, counts, s1, s2): the raw f64 moment rows [rows][n/2 + 1] of the newest `max_rows` blocks (default: all
        the ring holds), oldest first, with each row's absolute block index and its number of segments"""
        cap = self._cap(max_rows)
        b = self.n // 2 + 1
        idx, cnt, nr = np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.uint32), C.c_uint32()
        rows = [np.empty((max(cap, 1), b), np.float64) for _ in range(self._ROWS)]
        dp = C.POINTER(C.c_double)
        self._ck(self._f("stage_rows")(self._h, channel, stage, cap, idx.ctypes.data_as(C.POINTER(C.c_uint64)),
                                       cnt.ctypes.data_as(C.POINTER(C.c_uint32)), *(r.ctypes.data_as(dp) for r in rows), C.byref(nr)))
        m = nr.value
        return (idx[:m].copy(), cnt[:m].copy(), *(r[:m].copy() for r in rows))

    def _image_shape(self, rows):
        return (rows, self.n // 2 + 1)

    def image(self, channel, stage, max_rows=None):
        """(psd, sk, block_index, counts): float32 images [rows][n/2 + 1] of the newest `max_rows` blocks, oldest first, made on
        the device: psd is S1 scaled as the merged read-out scales an included stage of the row's count, sk the spectral
        kurtosis of the row's own segments (NaN below two segments and without power)"""
        cap = self._cap(max_rows)
        idx, cnt, nr = np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.uint32), C.c_uint32()
        psd, sk = np.empty(self._image_shape(max(cap, 1)), np.float32), np.empty(self._image_shape(max(cap, 1)), np.float32)
        self._ck(self._f("image")(self._h, channel, stage, cap, _fptr(psd), _fptr(sk), idx.ctypes.data_as(C.POINTER(C.c_uint64)),
                                  cnt.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(nr)))
        m = nr.value
        return psd[:m].copy(), sk[:m].copy(), idx[:m].copy(), cnt[:m].copy()

    def image_device(self, channel, stage, psd_ptr, sk_ptr, max_rows=None):
        """image() written into device memory: psd_ptr, sk_ptr are device addresses (a torch tensor's data_ptr()) of
        min(max_rows, depth) x the row shape of image() float32 each, either may be None.  Returns (block_index, counts) when the
        kernel has completed; their length is the number of rows written."""
        cap = self._cap(max_rows)
        idx, cnt, nr = np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.uint32), C.c_uint32()
        self._ck(self._f("image_device")(self._h, channel, stage, cap, C.c_void_p(psd_ptr) if psd_ptr else None,
                                         C.c_void_p(sk_ptr) if sk_ptr else None, idx.ctypes.data_as(C.POINTER(C.c_uint64)),
                                         cnt.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(nr)))
        m = nr.value
        return idx[:m].copy(), cnt[:m].copy()

    def block_span(self, stage, b):
        """range of the input samples block b of `stage` nominally covers:
        [b B hop 8^stage, ((b + 1) B - 1) hop 8^stage + n 8^stage).  The decimators' delay is not included."""
        return waterfall_block_span(self.n, self._table().overlap, self.block, stage, b)

    def _recent(self, channel, blocks, opts, nsides):
        ns = self.num_stages(channel)
        counts, avgs, pend = [], [], []
        rows = np.zeros((nsides, max(ns, 1), self.n // 2 + 1), np.float32)
        for k in range(ns):
            got = self.stage_rows(channel, k, blocks)
            counts.append(int(got[1].sum()))
            avgs.append(U32_MAX >> (3 * k) if 3 * k < 32 else 0)
            pend.append(self.stage_blocks(channel, k)["pending"])
            for s in range(nsides):
                rows[s, k] = got[2 + s].sum(axis=0)
        out = [stitch(self.n, counts, avgs, pend, rows[s, :ns], opts, window=self._table()) for s in range(nsides)]
        return [o[0] for o in out], out[0][1]

    def recent_psd(self, channel=0, blocks=1, opts=MergeOpts()):
        """(psd, breaks): the stitched log-resolution spectrum of the recent past: per stage the sum of its newest `blocks` ring
        rows (None: all it holds), merged by stitch() with the summed counts"""
        p, br = self._recent(channel, blocks, opts, 1)
        return p[0], br

    stats = _Stats.stats_read


class ZoomWaterfallCascadeBank(_ChannelCarriers, WaterfallCascadeBank):
    """`n_channels` independent zoom waterfall cascades (psdc_zwf_*): ZoomSkCascadeBank's carrier, mixer and two-sided stages with
    a ring of blocks a stage.  Fed as ZoomCascadeBank is.  Rows come per side, images as [rows][2][n/2 + 1] with side 0 the
    upper and side 1 the lower sideband."""

    _P = "psdc_zwf_"
    _ROWS = 4

    def __init__(self, n, n_channels=1, f0=None, ftw=None, block=64, depth=64, window=Window.HANN, device=0):
        super().__init__(n, n_channels, block, depth, window, device)
        if f0 is not None or ftw is not None:
            for c in range(n_channels):
                self.set_carrier(c, f0=f0, ftw=ftw)

    def stage_rows(self, channel, stage, max_rows=None):
        """(block_index, counts, s1_upper, s1_lower, s2_upper, s2_lower), as WaterfallCascadeBank.stage_rows per side"""
        return super().stage_rows(channel, stage, max_rows)

    def _image_shape(self, rows):
        return (rows, 2, self.n // 2 + 1)

    def recent_psd(self, channel=0, blocks=1, opts=MergeOpts()):
        """(upper, lower, breaks): WaterfallCascadeBank.recent_psd of each side, as ZoomCascadeBank.psd() lays them out"""
        p, br = self._recent(channel, blocks, opts, 2)
        return p[0], p[1], br


class WaterfallCascade(_Cascade):
    """One real stream: WaterfallCascade(n, block=64, depth=64).  image(stage) is that stage's PSD and SK against time."""

    _BANK = WaterfallCascadeBank

    def __init__(self, n, block=64, depth=64, window=Window.HANN, device=0):
        self.n, self.block, self.depth = n, block, depth
        self._b = self._BANK(n, 1, block=block, depth=depth, window=window, device=device)

    def process(self, x):
        self._b.process(0, x)

    def process_device(self, ptr, length, after=None):
        self._b.process_device(0, ptr, length, after)

    def stage_blocks(self, stage):
        return self._b.stage_blocks(0, stage)

    def stage_rows(self, stage, max_rows=None):
        return self._b.stage_rows(0, stage, max_rows)

    def image(self, stage, max_rows=None):
        return self._b.image(0, stage, max_rows)

    def image_device(self, stage, psd_ptr, sk_ptr, max_rows=None):
        return self._b.image_device(0, stage, psd_ptr, sk_ptr, max_rows)

    def block_span(self, stage, b):
        return self._b.block_span(stage, b)

    def recent_psd(self, blocks=1, opts=MergeOpts()):
        return self._b.recent_psd(0, blocks, opts)

    def reset(self):
        self._b.reset()

    def stats_read(self, reset=False):
        return self._b.stats_read(reset)

    stats = stats_read


class ZoomWaterfallCascade(_KeepsCarrier, WaterfallCascade):
    """One real stream around one carrier: ZoomWaterfallCascade(n, f0=0.2, block=64, depth=64) or (n, ftw=...).  `f0` is the
    frequency in use (ftw / 2^64).  reset() keeps the object's carrier."""

    _BANK = ZoomWaterfallCascadeBank

    def __init__(self, n, f0=None, ftw=None, phase0=0, block=64, depth=64, window=Window.HANN, device=0):
        super().__init__(n, block, depth, window, device)
        self._tune(f0, ftw, phase0)


def zoom_ampm_supported(n):
    """Whether ZoomAmPmCascade[Bank] and IqAmPmCascade[Bank] take the size n: a power of two 64 ... 4096 (the zoom object's)"""
    return 0 <= n < (1 << 32) and bool(lib().psdc_zampm_supported(n))


def am_pm_from_sidebands(upper, lower, comp, carrier):
    """(s_am, s_pm, s_ampm) in f64 from the two sideband rows, the complementary row comp = sum Z_k Z_(N-k) (all three in one
    normalisation) and the carrier's complex amplitude A.  With P = |A|^2, u = A^2 / |A|^2 and D = comp conj(u):
        s_am = ((U + L)/2 + Re D) / (2 P),   s_pm = ((U + L)/2 - Re D) / (2 P),   s_ampm = Im D / (2 P) + 1j (L - U) / (4 P)
    s_ampm = conj(a_k) phi_k is the AM-PM cross spectrum.  Only A^2 enters: the sign of A does not matter.
    The separation is a linear, small-modulation one for z = A (1 + a + i phi): phi^2 reads as AM at second order (-phi^2 / 2
    is amplitude).  The rows must come from a carrier that sat at the tuning word to within the reciprocal of the averaging time
    (carrier()'s lock says whether it did); bins 0 and 1 of a stage hold the carrier itself under a Hann window."""
    U, L = np.asarray(upper, np.float64), np.asarray(lower, np.float64)
    comp = np.asarray(comp, np.complex128)
    A = complex(carrier)
    P = abs(A) ** 2
    if not P > 0.0:
        raise PsdError(ERR_ARG, "am_pm_from_sidebands: the carrier's amplitude must not be 0")
    D = comp * np.conj(A * A / P)
    mean = 0.5 * (U + L)
    return (mean + D.real) / (2.0 * P), (mean - D.real) / (2.0 * P), D.imag / (2.0 * P) + 1j * (L - U) / (4.0 * P)


def carrier_from_rows(n, window_power, count, upper0, lower0, comp0):
    """(power, u, lock) of a carrier from bin 0 of a stage's raw rows: comp[0] = sum Z_0^2 = A^2 (sum win)^2 per segment, so
    u = comp0 / |comp0| = A^2 / |A|^2, power = |A|^2 = |comp0| / (count n^2 window_power) (window_power the window's coherent
    power gain, mean(win)^2: Window.power) and lock = |comp0| / sqrt(upper0 lower0): 1 for a carrier at the tuning word,
    towards 0 for one that turns during the average."""
    c = complex(comp0)
    mag = abs(c)
    if count < 1 or not mag > 0.0:
        raise PsdError(ERR_ARG, "carrier: no carrier in bin 0 (no average yet, or comp[0] == 0)")
    return mag / (float(count) * float(n) ** 2 * float(window_power)), c / mag, mag / float(np.sqrt(float(upper0) * float(lower0)))


class ZoomAmPmCascadeBank(_ChannelCarriers, _ChannelBank):
    """`n_channels` independent AM/PM cascades (psdc_zampm_*): ZoomCascadeBank's carrier, mixer and two-sided cascade, with the
    complementary spectrum comp[k] = sum Z_k Z_(N-k) kept beside upper and lower.  psd() is ZoomCascadeBank's; sidebands() adds
    comp, all in f64; am_pm() separates them into the amplitude noise, phase noise and AM-PM cross spectra of the carrier.
    Limits: the separation is a linear, small-modulation one (phi^2 reads as AM at second order); the carrier must sit at the
    tuning word to within the reciprocal of the averaging time -- carrier()'s lock says whether it does; bins 0 and 1 of every
    stage hold the carrier itself under Hann; a real stream's image at -2 f0 is where ZoomCascade has it.  Only f32 samples feed
    it: no stream frames, loss record or integer feeds yet."""

    _P = "psdc_zampm_"

    def _fresh(self, most=None):
        super()._fresh(most)
        self.detrend = Detrend.NONE

    def set_detrend(self, d):
        super().set_detrend(d)
        self.detrend = Detrend(int(d))

    def process(self, channel, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        self._ck(self._L.psdc_zampm_process(self._h, channel, _fptr(x), x.size))

    def process_device(self, channel, ptr, length, after=None):
        """ptr: device address of `length` f32 samples; after: a hipEvent_t handle recorded behind their producer, or None
        when it has completed.  The samples must stay unchanged until sync() or a read-out returns."""
        self._ck(self._L.psdc_zampm_process_device(self._h, channel, C.c_void_p(ptr), length, C.c_void_p(after) if after else None))

    def stage_rows(self, channel, stage):
        """(info, upper, lower, comp) of one stage: its raw accumulators, upper and lower f64, comp complex128"""
        b = self.n // 2 + 1
        st = _CStageStat()
        rows = [np.empty(b, np.float64) for _ in range(4)]
        dp = C.POINTER(C.c_double)
        self._ck(self._f("stage_rows")(self._h, channel, stage, C.byref(st), *(r.ctypes.data_as(dp) for r in rows)))
        return _stage_info(st), rows[0], rows[1], rows[2] + 1j * rows[3]

    def psd(self, channel=0, opts=MergeOpts()):
        """(upper, lower, breaks): the zoom read-out of rows 0 and 1, as ZoomCascadeBank.psd() returns it"""
        rows, br = self._merged(self._f("psd"), channel, opts, (1, 1))
        return (*rows, br)

    def sidebands(self, channel=0, opts=MergeOpts()):
        """(upper, lower, comp, breaks): all four rows merged as psd() merges, in f64 (comp complex128)"""
        rows, br = self._merged(self._f("sidebands"), channel, opts, (1, 1, 1, 1), np.float64)
        return rows[0], rows[1], rows[2] + 1j * rows[3], br

    def _window_power(self):
        return self.window.power if isinstance(self.window, WindowTable) else WindowTable._kind(self.n, self.window).power

    def carrier(self, channel=0):
        """(power, u, lock) of the channel's carrier, read from bin 0 of stage 0 (carrier_from_rows): power = |A|^2 of the
        baseband carrier (a real stream C cos(2 pi f0 j + th) has A = C/2 e^(i th)), u = A^2 / |A|^2, lock 1 for a carrier at the
        tuning word.  Raises unless detrend is none (a detrend removes the carrier from bin 0) and stage 0 has an average."""
        if self.detrend != Detrend.NONE:
            raise PsdError(ERR_ARG, "carrier: bin 0 holds the carrier under Detrend.NONE only; pass am_pm() the carrier")
        if self.num_stages(channel) < 1:
            raise PsdError(ERR_ARG, "carrier: stage 0 has no average yet")
        info, up, lo, comp = self.stage_rows(channel, 0)
        return carrier_from_rows(self.n, self._window_power(), info["count"], up[0], lo[0], comp[0])

    def am_pm(self, channel=0, carrier=None, opts=MergeOpts()):
        """(s_am, s_pm, s_ampm, breaks) in f64, in the one-sided normalisation of psd(): am_pm_from_sidebands of sidebands().
        carrier: the complex amplitude A of the baseband carrier, or None to take it from carrier() (Detrend.NONE only)."""
        if carrier is None:
            power, u, _ = self.carrier(channel)
            carrier = np.sqrt(power) * np.sqrt(complex(u))
        up, lo, comp, br = self.sidebands(channel, opts)
        return (*am_pm_from_sidebands(up, lo, comp, carrier), br)

    stats = _Stats.stats_read


class IqAmPmCascadeBank(ZoomAmPmCascadeBank):
    """`n_channels` independent IQ AM/PM cascades (psdc_iqampm_*): ZoomAmPmCascadeBank for streams that are complex already (a
    lock-in's or SDR's I/Q, Fls BI / BQ handed over as arrays), fed as IqCascadeBank is and turned by an optional carrier
    (default none)."""

    _P = "psdc_iqampm_"

    def process(self, channel, z):
        """z: a complex array (converted to complex64 and fed as (re, im) pairs: the interleaved route), or a pair (i, q) of
        real arrays of one length (the planar route)."""
        self._process_iq(channel, z)

    def process_device(self, channel, ptr, length, after=None):
        """ptr: device address of `length` (re, im) pairs of f32 (a complex64 tensor's memory; 8-byte aligned); the rest as
        ZoomAmPmCascadeBank.process_device"""
        self._ck(self._L.psdc_iqampm_process_interleaved_device(self._h, channel, C.c_void_p(ptr), length,
                                                                C.c_void_p(after) if after else None))

    def process_device_planar(self, channel, pi, pq, length, after=None):
        """pi, pq: device addresses of `length` f32 samples each, the I and the Q stream (process_device's rules)"""
        self._ck(self._L.psdc_iqampm_process_device(self._h, channel, C.c_void_p(pi), C.c_void_p(pq), length,
                                                    C.c_void_p(after) if after else None))


class ZoomAmPmCascade(_CarrierCascade):
    """One real stream around one carrier: ZoomAmPmCascade(n, f0=0.2) or ZoomAmPmCascade(n, ftw=...): psd() and sidebands(),
    carrier() and am_pm() (ZoomAmPmCascadeBank has the definitions and the limits).  `f0` is the frequency in use
    (ftw / 2^64).  reset() keeps the object's carrier."""

    _BANK = ZoomAmPmCascadeBank
    stats = _UnitCascade.stats_read

    def sidebands(self, opts=MergeOpts()):
        return self._b.sidebands(0, opts)

    def stage_rows(self, i):
        return self._b.stage_rows(0, i)

    def carrier(self):
        return self._b.carrier(0)

    def am_pm(self, carrier=None, opts=MergeOpts()):
        return self._b.am_pm(0, carrier, opts)


class IqAmPmCascade(ZoomAmPmCascade):
    """One complex stream: IqAmPmCascade(n) analyses it as it is, IqAmPmCascade(n, f0=0.2) or IqAmPmCascade(n, ftw=...) retunes
    it first.  process() takes a complex array or a pair (i, q), as IqCascade.process does."""

    _BANK = IqAmPmCascadeBank

    def process_device_planar(self, pi, pq, length, after=None):
        self._b.process_device_planar(0, pi, pq, length, after)


ZCSD_STEADY_LAUNCHES = 5  # PSDC_ZCSD_STEADY_LAUNCHES: two mixers; segments, decimators, fold + tails


def zcsd_supported(n):
    """True if a ZoomCsdCascadeBank of size n can be created (psdc_zcsd_supported).  Needs no GPU."""
    return 0 <= n < (1 << 32) and bool(lib().psdc_zcsd_supported(n))


class ZoomCsdCascadeBank(_SideCarriers, _FramesFeed, _PairBank):
    """`n_pairs` independent zoom cross cascades (psdc_zcsd_*): a pair is two real streams a and b, each mixed down from a
    carrier of its own (ZoomCascadeBank's tuning word and start phase) to I + i Q in front of the cascade.  Every stage keeps the
    two-sided auto spectra of both and their cross spectrum S_ab = conj(Z_a) Z_b (CsdCascade's sign), each as an `upper` row
    (f0 + f) and a `lower` row (f0 - f, the value at bin N - k, not conjugated).  Two receivers on one carrier: their own noise
    averages out of S_ab, the source's stays.  coherence(), transfer() and two_sided() take the rows of csd() as they are.

    Recipe (AM / PM separation): feed the SAME stream to both sides with the carriers ftw and -ftw, phase0 = 0.  S_bb upper is
    then S_aa lower and S_ab upper is conj(Z_k Z_-k), the term that separates amplitude from phase noise."""

    _P, _FP, _MAP = "psdc_zcsd_", "psdc_zoomcsdcascade_", staticmethod(pair_map)
    _ARG_WORDS = _Bank._ARG_WORDS + ("not supported",)

    def process(self, pair, x, y):
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.ascontiguousarray(y, dtype=np.float32)
        if x.size != y.size:
            raise PsdError(ERR_ARG, "x and y must have equal lengths")
        self._ck(self._L.psdc_zcsd_process(self._h, pair, _fptr(x), _fptr(y), x.size))

    def process_device(self, pair, px, py, length, after=None):
        """px, py: device addresses of `length` f32 samples each; after: a hipEvent_t handle recorded behind their producer, or
        None when it has completed.  The samples must stay unchanged until sync() or a read-out returns."""
        self._ck(self._L.psdc_zcsd_process_device(self._h, pair, C.c_void_p(px), C.c_void_p(py), length,
                                                  C.c_void_p(after) if after else None))

    def process_int(self, pair, x, y, scale=None):
        """x, y: 1-D int16 or int8 arrays of one dtype and length, fed as they are (ZoomCascadeBank.process_int, a side each)"""
        a, b = int_samples(x), int_samples(y)
        _same_kind(a, b)
        self._ck(self._L.psdc_int_zcsd_process(self._h, pair, a[0].ctypes.data_as(C.c_void_p), b[0].ctypes.data_as(C.c_void_p),
                                               int(a[1]), a[2] if scale is None else float(scale), a[0].size))

    def process_int_device(self, pair, px, py, length, kind, scale=None, after=None):
        """px, py: device addresses of `length` integers of SampleKind `kind` each; the rest as process_device"""
        kind, scale = _int_scale(kind, scale)
        self._ck(self._L.psdc_int_zcsd_process_device(self._h, pair, C.c_void_p(px), C.c_void_p(py), kind, scale, length,
                                                      C.c_void_p(after) if after else None))

    def process_frames(self, data, frame_size, pairs):
        """Stream frames of any of the four payload formats (bytes-like holding whole frames) into the pairs: pairs[p] is (x, y),
        the traces sides a and b of pair p take of every frame (indices or TRACE_NAMES labels, pair_map), or None to leave the
        pair unfed; a trace may feed several sides, both sides of one pair included.  The frames are decoded and mixed on the
        device in one kernel; two sides with one carrier share the oscillator.  Returns the number of frames ingested; a bad
        frame raises FrameError after the frames before it were ingested."""
        return self._frames(data, frame_size, pairs)

    def process_frames_device(self, ptr, frame_size, n_frames, pairs, after=None):
        """process_frames for frames resident in device memory at address `ptr`; after: a hipEvent_t handle recorded behind
        their producer, or None when it has completed.  The payloads must stay unchanged until sync() or a read-out returns."""
        return self._frames_device(ptr, frame_size, n_frames, pairs, after)

    def stage_spectra(self, pair, stage):
        """(info, rows) of one stage's raw accumulators: rows (8, n/2 + 1) in the layout of include/psdcascade.h -- S_aa upper,
        lower; S_bb upper, lower; Re S_ab upper, lower; Im S_ab upper, lower."""
        st = _CStageStat()
        rows = np.empty((8, self.n // 2 + 1), np.float32)
        self._ck(self._f("stage_spectra")(self._h, pair, stage, C.byref(st), _fptr(rows)))
        return _stage_info(st), rows

    def csd(self, pair=0, opts=MergeOpts()):
        """(saa_up, saa_lo, sbb_up, sbb_lo, sab_up, sab_lo, breaks): PsdCascade::psd of every row, sab complex;
        Break.frequencies(breaks) are the offsets of all."""
        rows, br = self._merged(self._f("csd"), pair, opts, (1, 1, 1, 1, 2, 2))
        return (*rows[:4], *((a[0::2] + 1j * a[1::2]).astype(np.complex64) for a in rows[4:]), br)


class ZoomCsdCascade(_PairCarrierCascade):
    """One pair around a carrier: ZoomCsdCascade(n, f0=0.2) or ZoomCsdCascade(n, ftw=...) sets both sides; set_carrier(side=...)
    sets one.  reset() keeps the object's carriers."""

    _BANK = ZoomCsdCascadeBank

    def process_int(self, x, y, scale=None):
        self._b.process_int(0, x, y, scale)

    def process_int_device(self, px, py, length, kind, scale=None, after=None):
        self._b.process_int_device(0, px, py, length, kind, scale, after)

    def process_frames(self, data, frame_size, pair):
        """pair: (x, y), the traces of the frames the two streams are (ZoomCsdCascadeBank.process_frames)"""
        return self._b.process_frames(data, frame_size, [pair])

    def process_frames_device(self, ptr, frame_size, n_frames, pair, after=None):
        return self._b.process_frames_device(ptr, frame_size, n_frames, [pair], after)

    def loss(self, reset=False):
        return self._b.loss(reset)

    def stage_spectra(self, i):
        return self._b.stage_spectra(0, i)


IQCSD_STEADY_LAUNCHES = 4  # PSDC_IQCSD_STEADY_LAUNCHES: pair mixer; segments, decimators, fold + tails


def iqcsd_supported(n):
    """True if an IqCsdCascadeBank of size n can be created (psdc_iqcsd_supported: the zoom cross object's sizes).  Needs no GPU."""
    return 0 <= n < (1 << 32) and bool(lib().psdc_iqcsd_supported(n))


def iq_pair_map(pairs, n_pairs):
    """The map psdc_iqcsd_process_frames[_device] take, from `pairs`: entry p is ((ia, qa), (ib, qb)), the traces the two sides of
    pair p take as I and Q -- indices or TRACE_NAMES labels (trace_index), e.g. (("BI", "BQ"), ("AR", "AP")) --, or None, or a
    pair whose four entries are all None (pair p not fed); pairs past the end of the list are not fed.  A map that feeds no pair,
    a pair with one to three None, an index outside 0 ... 3 and an unknown label are ERR_ARG here, before the library sees the
    call."""
    pairs = list(pairs)
    if len(pairs) > n_pairs:
        raise PsdError(ERR_ARG, f"{len(pairs)} entries for a bank of {n_pairs} pairs")
    m = np.full(4 * n_pairs, TRACE_NONE, np.uint32)
    for p, ab in enumerate(pairs):
        if ab is None:
            continue
        ok = isinstance(ab, (tuple, list)) and len(ab) == 2 and all(isinstance(s, (tuple, list)) and len(s) == 2 for s in ab)
        if not ok:
            raise PsdError(ERR_ARG, f"pair {p} needs ((ia, qa), (ib, qb))")
        four = [ab[0][0], ab[0][1], ab[1][0], ab[1][1]]
        none = sum(t is None for t in four)
        if none == 4:
            continue
        if none:
            raise PsdError(ERR_ARG, f"pair {p} names None for some of its traces only")
        for c, t in enumerate(four):
            i = trace_index(t)
            if not 0 <= i < 4:
                raise PsdError(ERR_ARG, f"pair {p} names trace {i} (frames carry at most 4)")
            m[4 * p + c] = i
    if not np.any(m != TRACE_NONE):
        raise PsdError(ERR_ARG, "the map feeds no pair")
    return m


class IqCsdCascadeBank(ZoomCsdCascadeBank):
    """`n_pairs` independent IQ cross cascades (psdc_iqcsd_*): a pair is two streams that are complex already, a = I_a + i Q_a
    and b = I_b + i Q_b, each turned by a carrier of its own (default none: ftw = 0, phase0 = 0) in one pair mixer launch in front
    of the zoom cross object's cascade.  Every stage keeps the two-sided auto spectra of both and their cross spectrum
    S_ab = conj(Z_a) Z_b, each as an `upper` row (offsets f >= 0) and a `lower` row (-f, the value at bin N - k, not
    conjugated), exactly as ZoomCsdCascadeBank does.  coherence(), transfer() and two_sided() take the rows of csd() as they are."""

    _P, _FP, _MAP = "psdc_iqcsd_", "psdc_iqcsd_", staticmethod(iq_pair_map)
    _SIDES = "0: stream a, 1: stream b"

    def process(self, pair, za, zb):
        """za, zb: two complex arrays of one length (converted to complex64 and fed as (re, im) pairs: the interleaved route), or
        two pairs (ia, qa), (ib, qb) of real arrays of one length (the planar route)."""
        self._process_iq_pair(pair, za, zb)

    def process_device(self, pair, pa, pb, length, after=None):
        """pa, pb: device addresses of `length` (re, im) pairs of f32 each (two complex64 tensors' memory; 8-byte aligned); after:
        a hipEvent_t handle recorded behind their producer, or None when it has completed.  The samples must stay unchanged
        until sync() or a read-out returns."""
        self._ck(self._L.psdc_iqcsd_process_interleaved_device(self._h, pair, C.c_void_p(pa), C.c_void_p(pb), length,
                                                               C.c_void_p(after) if after else None))

    def process_int(self, pair, za, zb, scale=None):
        """za, zb: C-contiguous int16 or int8 arrays of shape (len, 2) of one dtype and length, the (re, im) rows of each side, fed
        as they are (IqCascadeBank.process_int, a side each)"""
        a, b = int_pairs(za), int_pairs(zb)
        _same_kind(a, b)
        self._ck(self._L.psdc_int_iqcsd_process(self._h, pair, a[0].ctypes.data_as(C.c_void_p), b[0].ctypes.data_as(C.c_void_p),
                                                int(a[1]), a[2] if scale is None else float(scale), a[0].shape[0]))

    def process_int_device(self, pair, pa, pb, length, kind, scale=None, after=None):
        """pa, pb: device addresses of `length` (re, im) integer pairs of SampleKind `kind` each; the rest as process_device"""
        kind, scale = _int_scale(kind, scale)
        self._ck(self._L.psdc_int_iqcsd_process_device(self._h, pair, C.c_void_p(pa), C.c_void_p(pb), kind, scale, length,
                                                       C.c_void_p(after) if after else None))

    def process_device_planar(self, pair, pia, pqa, pib, pqb, length, after=None):
        """pia, pqa, pib, pqb: device addresses of `length` f32 samples each, the I and Q streams of side a and of side b
        (process_device's rules)"""
        self._ck(self._L.psdc_iqcsd_process_device(self._h, pair, C.c_void_p(pia), C.c_void_p(pqa), C.c_void_p(pib),
                                                   C.c_void_p(pqb), length, C.c_void_p(after) if after else None))

    def process_frames(self, data, frame_size, pairs):
        """Stream frames of any of the four payload formats (bytes-like holding whole frames) into the pairs: pairs[p] is
        ((ia, qa), (ib, qb)), the traces the two sides of pair p take as I and Q of every frame (indices or TRACE_NAMES labels,
        iq_pair_map), or None to leave the pair unfed; a trace may feed any number of sides.  The frames are decoded and mixed on
        the device in one kernel; two sides with one carrier share the oscillator.  Returns the number of frames ingested; a
        bad frame raises FrameError after the frames before it were ingested."""
        return self._frames(data, frame_size, pairs)

    stats = _Stats.stats_read


class IqCsdCascade(ZoomCsdCascade):
    """One pair of complex streams: IqCsdCascade(n) analyses them as they are, IqCsdCascade(n, f0=0.2) or IqCsdCascade(n, ftw=...)
    retunes both sides first; set_carrier(side=...) sets one.  reset() keeps the object's carriers."""

    _BANK = IqCsdCascadeBank

    def process(self, za, zb):
        """za, zb: two complex arrays, or two pairs (i, q) (IqCsdCascadeBank.process)"""
        self._b.process(0, za, zb)

    def process_device(self, pa, pb, length, after=None):
        self._b.process_device(0, pa, pb, length, after)

    def process_int(self, za, zb, scale=None):
        self._b.process_int(0, za, zb, scale)

    def process_int_device(self, pa, pb, length, kind, scale=None, after=None):
        self._b.process_int_device(0, pa, pb, length, kind, scale, after)

    def process_device_planar(self, pia, pqa, pib, pqb, length, after=None):
        self._b.process_device_planar(0, pia, pqa, pib, pqb, length, after)

    def process_frames(self, data, frame_size, pair):
        """pair: ((ia, qa), (ib, qb)), the traces of the frames the two streams are (IqCsdCascadeBank.process_frames)"""
        return self._b.process_frames(data, frame_size, [pair])

    stats = _UnitCascade.stats_read


def zoom_ampm_cross_supported(n):
    """Whether ZoomAmPmCsdCascade[Bank] and IqAmPmCsdCascade[Bank] take the size n: the zoom cross object's sizes (the twelve-row
    kernel needs no scratch memory at any of them).  Needs no GPU."""
    return 0 <= n < (1 << 32) and bool(lib().psdc_zxampm_supported(n))


def carriers_from_rows(n, window_power, count, saa_up0, sbb_up0, sbb_lo0, sab_up0, cab0):
    """(p_ab, w, q, lock_w, lock_q) of a pair's carriers from bin 0 of a stage's raw rows.  With v_x = A_x / |A_x|:
    sab_up[0] = P w count n^2 window_power and cab[0] = P q count n^2 window_power, where P = |A_a| |A_b|, w = conj(v_a) v_b and
    q = v_a v_b; so p_ab = |sab_up0| / (count n^2 window_power), w = sab_up0 / |sab_up0|, q = cab0 / |cab0|,
    lock_w = |sab_up0| / sqrt(saa_up0 sbb_up0) and lock_q = |cab0| / sqrt(saa_up0 sbb_lo0): 1 for carriers at their tuning
    words, towards 0 when one turns against the other (lock_w) or against its tuning word (lock_q) during the average."""
    u, c = complex(sab_up0), complex(cab0)
    if count < 1 or not abs(u) > 0.0 or not abs(c) > 0.0:
        raise PsdError(ERR_ARG, "carriers: no carriers in bin 0 (no average yet, or sab_up[0] == 0 or cab[0] == 0)")
    saa, sbu, sbl = float(saa_up0), float(sbb_up0), float(sbb_lo0)
    return (abs(u) / (float(count) * float(n) ** 2 * float(window_power)), u / abs(u), c / abs(c),
            abs(u) / float(np.sqrt(saa * sbu)), abs(c) / float(np.sqrt(saa * sbl)))


def am_pm_cross_from_sidebands(sab_up, sab_lo, cab, cba, p_ab, w, q):
    """(s_am, s_pm, s_am_pm, s_pm_am), complex128, from the cross rows of a pair (all four in one normalisation) and the carriers'
    p_ab = |A_a| |A_b|, w = conj(v_a) v_b, q = v_a v_b (v_x = A_x / |A_x|).  With U = sab_up, L = sab_lo, T1 = U conj(w),
    T2 = conj(cab) q, T3 = cba conj(q), T4 = conj(L) w:
        s_am    = conj(a_a) a_b     = ( T1 + T2 + T3 + T4) / (4 P)      s_pm    = conj(phi_a) phi_b = (T1 - T2 - T3 + T4) / (4 P)
        s_am_pm = conj(a_a) phi_b   = ( T1 - T2 + T3 - T4) / (4i P)     s_pm_am = conj(phi_a) a_b   = i (T1 + T2 - T3 - T4) / (4 P)
    The separation is a linear, small-modulation one for z_x = A_x (1 + a_x + i phi_x): phi^2 reads as AM at second order.  The
    rows must come from carriers that sat at their tuning words to within the reciprocal of the averaging time (carriers()'s
    locks say whether they did); bins 0 and 1 of a stage hold the carriers themselves under a Hann window."""
    U, L = np.asarray(sab_up, np.complex128), np.asarray(sab_lo, np.complex128)
    cab, cba = np.asarray(cab, np.complex128), np.asarray(cba, np.complex128)
    P, w, q = float(p_ab), complex(w), complex(q)
    if not P > 0.0 or not abs(w) > 0.0 or not abs(q) > 0.0:
        raise PsdError(ERR_ARG, "am_pm_cross_from_sidebands: p_ab, w and q must not be 0")
    w, q = w / abs(w), q / abs(q)
    t1, t2, t3, t4 = U * np.conj(w), np.conj(cab) * q, cba * np.conj(q), np.conj(L) * w
    return ((t1 + t2 + t3 + t4) / (4.0 * P), (t1 - t2 - t3 + t4) / (4.0 * P), (t1 - t2 + t3 - t4) / (4.0j * P),
            1j * (t1 + t2 - t3 - t4) / (4.0 * P))


class ZoomAmPmCsdCascadeBank(_SideCarriers, _PairBank):
    """`n_pairs` independent AM/PM cross cascades (psdc_zxampm_*): ZoomCsdCascadeBank's pair -- two real streams a and b, each
    mixed down from a carrier of its own -- on one transform a channel and segment, with the two complementary cross spectra
    cab[k] = sum Z_a[k] Z_b[N-k] and cba[k] = sum Z_a[N-k] Z_b[k] (products WITHOUT a conjugate) kept beside the zoom cross
    object's eight rows.  csd() is ZoomCsdCascadeBank's; sidebands() adds cab and cba, all in f64; am_pm_cross() separates them into
    the cross spectra of the two channels' amplitude and phase modulation: what both channels share stays, each channel's own
    noise averages down as 1 / sqrt(count).
    Limits (those of ZoomAmPmCascadeBank): the separation is a linear, small-modulation one (phi^2 reads as AM at second order);
    both carriers must sit at their tuning words to within the reciprocal of the averaging time -- carriers()'s locks say whether
    they do; bins 0 and 1 of every stage hold the carriers themselves under Hann.  Only f32 samples feed it: no stream frames,
    loss record or integer feeds."""

    _P = "psdc_zxampm_"
    _ARG_WORDS = _Bank._ARG_WORDS + ("not supported",)
    _CARRIERS = "carriers_set"   # (carriers() is the read-out of the carriers themselves)

    def _fresh(self, most=None):
        super()._fresh(most)
        self.detrend = Detrend.NONE

    def set_detrend(self, d):
        super().set_detrend(d)
        self.detrend = Detrend(int(d))

    def process(self, pair, x, y):
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.ascontiguousarray(y, dtype=np.float32)
        if x.size != y.size:
            raise PsdError(ERR_ARG, "x and y must have equal lengths")
        self._ck(self._L.psdc_zxampm_process(self._h, pair, _fptr(x), _fptr(y), x.size))

    def process_device(self, pair, px, py, length, after=None):
        """px, py: device addresses of `length` f32 samples each; after: a hipEvent_t handle recorded behind their producer, or
        None when it has completed.  The samples must stay unchanged until sync() or a read-out returns."""
        self._ck(self._L.psdc_zxampm_process_device(self._h, pair, C.c_void_p(px), C.c_void_p(py), length,
                                                    C.c_void_p(after) if after else None))

    def stage_rows(self, pair, stage):
        """(info, rows) of one stage's raw f64 accumulators: rows (12, n/2 + 1) in the layout of include/psdcascade.h -- the zoom
        cross object's eight, then Re cab, Im cab, Re cba, Im cba"""
        st = _CStageStat()
        rows = np.empty((12, self.n // 2 + 1), np.float64)
        self._ck(self._f("stage_rows")(self._h, pair, stage, C.byref(st), rows.ctypes.data_as(C.POINTER(C.c_double))))
        return _stage_info(st), rows

    def _twelve(self, pair, opts):
        return self._merged(self._f("sidebands"), pair, opts, 12, np.float64)

    def sidebands(self, pair=0, opts=MergeOpts()):
        """(saa_up, saa_lo, sbb_up, sbb_lo, sab_up, sab_lo, cab, cba, breaks): all twelve rows merged with one set of Breaks, in
        f64 (the last four complex128)"""
        r, br = self._twelve(pair, opts)
        return (r[0].copy(), r[1].copy(), r[2].copy(), r[3].copy(), r[4] + 1j * r[6], r[5] + 1j * r[7], r[8] + 1j * r[9],
                r[10] + 1j * r[11], br)

    def csd(self, pair=0, opts=MergeOpts()):
        """(saa_up, saa_lo, sbb_up, sbb_lo, sab_up, sab_lo, breaks): ZoomCsdCascadeBank.csd()'s tuple (f32, sab complex64), taken
        from rows 0 ... 7"""
        r, br = self._twelve(pair, opts)
        return (*(r[i].astype(np.float32) for i in range(4)), (r[4] + 1j * r[6]).astype(np.complex64),
                (r[5] + 1j * r[7]).astype(np.complex64), br)

    def _window_power(self):
        return self.window.power if isinstance(self.window, WindowTable) else WindowTable._kind(self.n, self.window).power

    def carriers(self, pair=0):
        """(p_ab, w, q, lock_w, lock_q) of the pair's carriers, read from bin 0 of stage 0 (carriers_from_rows).  Raises unless
        detrend is none (a detrend removes the carriers from bin 0) and stage 0 has an average."""
        if self.detrend != Detrend.NONE:
            raise PsdError(ERR_ARG, "carriers: bin 0 holds the carriers under Detrend.NONE only; pass am_pm_cross() the carriers")
        if self.num_stages(pair) < 1:
            raise PsdError(ERR_ARG, "carriers: stage 0 has no average yet")
        info, r = self.stage_rows(pair, 0)
        return carriers_from_rows(self.n, self._window_power(), info["count"], r[0, 0], r[2, 0], r[3, 0], r[4, 0] + 1j * r[6, 0],
                                  r[8, 0] + 1j * r[9, 0])

    def am_pm_cross(self, pair=0, carriers=None, opts=MergeOpts()):
        """(s_am, s_pm, s_am_pm, s_pm_am, breaks), complex128, in the one-sided normalisation of psd(): am_pm_cross_from_sidebands
        of sidebands().  carriers: (p_ab, w, q), or None to take them from carriers() (Detrend.NONE only)."""
        if carriers is None:
            carriers = self.carriers(pair)
        p_ab, w, q = carriers[:3]
        sb = self.sidebands(pair, opts)
        return (*am_pm_cross_from_sidebands(sb[4], sb[5], sb[6], sb[7], p_ab, w, q), sb[8])


class IqAmPmCsdCascadeBank(ZoomAmPmCsdCascadeBank):
    """`n_pairs` independent IQ AM/PM cross cascades (psdc_iqxampm_*): ZoomAmPmCsdCascadeBank for two streams that are complex
    already (two lock-ins' or SDRs' I/Q), fed as IqCsdCascadeBank is and turned by an optional carrier a side (default none)."""

    _P = "psdc_iqxampm_"

    def process(self, pair, za, zb):
        """za, zb: two complex arrays of one length (converted to complex64 and fed as (re, im) pairs: the interleaved route), or
        two pairs (ia, qa), (ib, qb) of real arrays of one length (the planar route)."""
        self._process_iq_pair(pair, za, zb)

    def process_device(self, pair, pa, pb, length, after=None):
        """pa, pb: device addresses of `length` (re, im) pairs of f32 each (two complex64 tensors' memory; 8-byte aligned); the
        rest as ZoomAmPmCsdCascadeBank.process_device"""
        self._ck(self._L.psdc_iqxampm_process_interleaved_device(self._h, pair, C.c_void_p(pa), C.c_void_p(pb), length,
                                                                 C.c_void_p(after) if after else None))

    def process_device_planar(self, pair, pia, pqa, pib, pqb, length, after=None):
        """pia, pqa, pib, pqb: device addresses of `length` f32 samples each, the I and Q streams of side a and of side b"""
        self._ck(self._L.psdc_iqxampm_process_device(self._h, pair, C.c_void_p(pia), C.c_void_p(pqa), C.c_void_p(pib),
                                                     C.c_void_p(pqb), length, C.c_void_p(after) if after else None))


class ZoomAmPmCsdCascade(_PairCarrierCascade):
    """One pair around a carrier: ZoomAmPmCsdCascade(n, f0=0.2) or ZoomAmPmCsdCascade(n, ftw=...) sets both sides;
    set_carrier(side=...) sets one.  csd(), sidebands(), carriers() and am_pm_cross() (ZoomAmPmCsdCascadeBank has the definitions
    and the limits).  reset() keeps the object's carriers."""

    _BANK = ZoomAmPmCsdCascadeBank

    def sidebands(self, opts=MergeOpts()):
        return self._b.sidebands(0, opts)

    def carriers(self):
        return self._b.carriers(0)

    def am_pm_cross(self, carriers=None, opts=MergeOpts()):
        return self._b.am_pm_cross(0, carriers, opts)

    def stage_rows(self, i):
        return self._b.stage_rows(0, i)


class IqAmPmCsdCascade(ZoomAmPmCsdCascade):
    """One pair of complex streams: IqAmPmCsdCascade(n) analyses them as they are, IqAmPmCsdCascade(n, f0=0.2) or
    IqAmPmCsdCascade(n, ftw=...) retunes both sides first.  process() takes two complex arrays or two pairs (i, q), as
    IqCsdCascade.process does."""

    _BANK = IqAmPmCsdCascadeBank

    def process_device_planar(self, pia, pqa, pib, pqb, length, after=None):
        self._b.process_device_planar(0, pia, pqa, pib, pqb, length, after)


def coherence(sxx, syy, sxy):
    """|Sxy|^2 / (Sxx Syy), NaN where the denominator is zero."""
    sxx, syy = np.asarray(sxx, np.float64), np.asarray(syy, np.float64)
    num = np.abs(np.asarray(sxy, np.complex128)) ** 2
    den = sxx * syy
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den != 0, num / np.where(den != 0, den, 1.0), np.nan)


def transfer(sxx, sxy):
    """H1 = Sxy / Sxx (complex), NaN where Sxx is zero."""
    sxx = np.asarray(sxx, np.float64)
    sxy = np.asarray(sxy, np.complex128)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(sxx != 0, sxy / np.where(sxx != 0, sxx, 1.0), np.nan + 0j)


def mimo_transfer(S, inputs, outputs):
    """The multi-input H1 of a spectral matrix S (m, m, bins): H of shape (len(outputs), len(inputs), bins) solving
    S[inputs, inputs] H^T = S[inputs, outputs] per bin, in complex128.  Unlike the single-input transfer() it is unbiased when
    the inputs are correlated; with one input it equals transfer().  NaN where the input matrix is singular."""
    S = np.asarray(S, np.complex128)
    ii, oo = list(inputs), list(outputs)
    sxx = np.moveaxis(S[np.ix_(ii, ii)], 2, 0)  # (bins, ni, ni)
    sxy = np.moveaxis(S[np.ix_(ii, oo)], 2, 0)  # (bins, ni, no)
    H = np.full((len(oo), len(ii), S.shape[2]), np.nan + 0j, np.complex128)
    for k in range(S.shape[2]):
        try:
            H[:, :, k] = np.linalg.solve(sxx[k], sxy[k]).T
        except np.linalg.LinAlgError:
            pass
    return H


def multiple_coherence(S, inputs, output):
    """S_xy^H S_xx^-1 S_xy / S_yy per bin (real, in [0, 1] up to rounding): the share of the output's power the inputs explain
    together.  With one input it equals coherence().  NaN where S_yy is zero or the input matrix is singular."""
    S = np.asarray(S, np.complex128)
    ii = list(inputs)
    sxx = np.moveaxis(S[np.ix_(ii, ii)], 2, 0)
    sxy = np.moveaxis(S[np.ix_(ii, [output])], 2, 0)
    syy = S[output, output].real
    out = np.full(S.shape[2], np.nan)
    for k in range(S.shape[2]):
        if syy[k] == 0:
            continue
        try:
            out[k] = (np.conj(sxy[k]).T @ np.linalg.solve(sxx[k], sxy[k]))[0, 0].real / syy[k]
        except np.linalg.LinAlgError:
            pass
    return out


class Psd:
    """One stage: `Psd<N>` with the `PsdStage` trait (src/psd.rs:122-288).

        s = Psd(512)                     Psd::<N>::new(fft, Arc::new(Window::hann()))   src/psd.rs:137
        y = s.process(x)                 PsdStage::process(&x, &mut y) -> &mut y[..n]   src/psd.rs:196-269
        s.spectrum(), s.gain(), s.count(), s.buf()                                      src/psd.rs:271-287
    """

    def __init__(self, n, window=Window.HANN, device=0, _handle=None):
        self.n, self.window, self.device = n, window, device
        self._L = lib()
        if _handle is not None:
            self._s = _handle
        elif isinstance(window, WindowTable):
            w = np.ascontiguousarray(window.win, dtype=np.float32)
            if w.size != n:
                raise PsdError(ERR_ARG, "window table length != n")
            self._s = self._L.psdc_stage_create_window(n, _fptr(w), window.power, window.nenbw, window.overlap, device)
        else:
            self._s = self._L.psdc_stage_create(n, int(window), device)
        if not self._s:
            _raise(ERR_DEVICE)

    @staticmethod
    def new(fft_len, win, n=None, device=0):
        """`Psd::<N>::new(fft, win)` (src/psd.rs:137-152): `fft_len` stands for the plan (`fft.len()`), `win` is a
        WindowTable; assert_eq!(N, fft.len()) (src/psd.rs:139) is kept."""
        n = len(win.win) if n is None else n
        if fft_len != n:
            raise PsdError(ERR_ARG, f"assertion failed: N == fft.len() ({n} vs {fft_len}) (src/psd.rs:139)")
        return Psd(n, win, device)

    def close(self):
        if getattr(self, "_s", None):
            self._L.psdc_stage_destroy(self._s)
            self._s = None

    __del__ = close

    def _ck(self, rc):
        if rc < 0:
            msg = self._L.psdc_stage_last_error(self._s)
            raise PsdError(rc, msg.decode() if msg else "")
        return rc

    def clone(self):
        h = self._L.psdc_stage_clone(self._s)
        if not h:
            _raise(ERR_DEVICE)
        return Psd(self.n, self.window, self.device, _handle=h)

    def set_avg(self, avg):
        self._ck(self._L.psdc_stage_set_avg(self._s, avg))

    def set_detrend(self, d):
        self._ck(self._L.psdc_stage_set_detrend(self._s, int(d)))

    def process(self, x, y=None):
        """Returns the written prefix of y (allocated with x.len()/8 + N/8 items when not given)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if y is None:
            y = np.empty(x.size // 8 + self.n // 8, dtype=np.float32)
        assert y.dtype == np.float32 and y.flags.c_contiguous
        m = C.c_size_t()
        self._ck(self._L.psdc_stage_process(self._s, _fptr(x), x.size, _fptr(y), y.size, C.byref(m)))
        return y[:m.value]

    def process_device(self, x_ptr, length, y_ptr, cap):
        m = C.c_size_t()
        self._ck(self._L.psdc_stage_process_device(self._s, C.c_void_p(x_ptr), length, C.c_void_p(y_ptr), cap,
                                                   C.byref(m)))
        return m.value

    def spectrum(self):
        out = np.empty(self.n // 2 + 1, dtype=np.float32)
        self._ck(self._L.psdc_stage_get_spectrum(self._s, _fptr(out)))
        return out

    def count(self):
        c = C.c_uint32()
        self._ck(self._L.psdc_stage_get_count(self._s, C.byref(c)))
        return c.value

    def gain(self):
        g = C.c_float()
        self._ck(self._L.psdc_stage_get_gain(self._s, C.byref(g)))
        return g.value

    def buf(self):
        ln = C.c_size_t()
        self._ck(self._L.psdc_stage_get_buf(self._s, None, 0, C.byref(ln)))
        out = np.empty(ln.value, dtype=np.float32)
        if ln.value:
            self._ck(self._L.psdc_stage_get_buf(self._s, _fptr(out), out.size, C.byref(ln)))
        return out


# ---- pure host helpers (no device) -----------------------------------------

def hbf_response_length(depth=3):
    """idsp::hbf::hbf_dec_response_length (src/psd.rs:149,622)."""
    return lib().psdc_hbf_response_length(depth)


def plan_counts(n, total, window=Window.HANN, cap=32):
    """Closed-form (received, segments, pending) per stage after `total` samples."""
    r = (C.c_uint64 * cap)()
    s = (C.c_uint64 * cap)()
    p = (C.c_uint64 * cap)()
    k = lib().psdc_plan_counts(n, int(window), total, cap, r, s, p)
    if k < 0:
        _raise(k)
    return [(int(r[i]), int(s[i]), int(p[i])) for i in range(min(k, cap))]


def stitch(n, counts, avgs, pendings, spectra, opts=MergeOpts(), window=Window.HANN):
    """PsdCascade::psd (src/psd.rs:479-543) on gathered per-stage data (stage 0 first).  `counts` may exceed
    u32 (the library counts in 64 bits); `window` is a kind or a WindowTable."""
    L = lib()
    ns = len(counts)
    if isinstance(window, WindowTable) or any(int(c) > U32_MAX for c in counts):
        wt = window if isinstance(window, WindowTable) else WindowTable._kind(n, window)
        c64 = (C.c_uint64 * max(1, ns))(*[int(c) for c in counts])
        aa = (C.c_uint32 * max(1, ns))(*avgs)
        pp = (C.c_uint64 * max(1, ns))(*pendings)
        sp = np.ascontiguousarray(spectra, dtype=np.float32).reshape(ns, n // 2 + 1) if ns else np.zeros((1, 1), np.float32)
        out = np.empty(max(1, ns * (n // 2 + 1)), dtype=np.float32)
        br = (_CBreak * max(1, ns))()
        plen, nb = C.c_size_t(), C.c_size_t()
        rc = L.psdc_stitch_window(n, wt.power, wt.nenbw, wt.overlap, ns, c64, aa, pp, _fptr(sp), int(opts.keep_overlap),
                                  opts.min_count, int(opts.keep_transition_band), _fptr(out), out.size, C.byref(plen), br,
                                  ns, C.byref(nb))
        if rc < 0:
            _raise(rc)
        return out[:plen.value].copy(), [Break._from_c(br[i]) for i in range(nb.value)]
    cc = (C.c_uint32 * max(1, ns))(*counts)
    aa = (C.c_uint32 * max(1, ns))(*avgs)
    pp = (C.c_uint64 * max(1, ns))(*pendings)
    sp = np.ascontiguousarray(spectra, dtype=np.float32).reshape(ns, n // 2 + 1) if ns else np.zeros((1, 1), np.float32)
    out = np.empty(max(1, ns * (n // 2 + 1)), dtype=np.float32)
    br = (_CBreak * max(1, ns))()
    plen, nb = C.c_size_t(), C.c_size_t()
    rc = L.psdc_stitch(n, int(window), ns, cc, aa, pp, _fptr(sp), int(opts.keep_overlap),
                       opts.min_count, int(opts.keep_transition_band), _fptr(out), out.size,
                       C.byref(plen), br, ns, C.byref(nb))
    if rc < 0:
        _raise(rc)
    return out[:plen.value].copy(), [Break._from_c(br[i]) for i in range(nb.value)]


def readout_bytes(n, n_channels):
    return lib().psdc_readout_bytes(n, n_channels)


def pack_record(n, channels, window=Window.HANN, rows=None):
    """A packed read-out record (psdc_pack_init / psdc_pack_channel, pure host) from stage data held by the caller:
    channels = [(counts, avgs, pendings, spectra[ns, n/2+1]) ...]; `rows` >= len(channels) pads with empty channels."""
    L = lib()
    wt = window if isinstance(window, WindowTable) else WindowTable._kind(n, window)
    rows = max(rows or 0, len(channels))
    buf = np.empty(L.psdc_readout_bytes(n, rows), dtype=np.uint8)
    rc = L.psdc_pack_init(buf.ctypes.data_as(C.c_void_p), buf.size, n, wt.power, wt.nenbw, wt.overlap, rows)
    if rc < 0:
        _raise(rc)
    for c, (counts, avgs, pend, sp) in enumerate(channels):
        ns = len(counts)
        sp = np.ascontiguousarray(sp, dtype=np.float32).reshape(ns, n // 2 + 1) if ns else np.zeros((1, 1), np.float32)
        rc = L.psdc_pack_channel(buf.ctypes.data_as(C.c_void_p), buf.size, c, ns,
                                 (C.c_uint64 * max(1, ns))(*[int(v) for v in counts]),
                                 (C.c_uint32 * max(1, ns))(*[int(v) for v in avgs]),
                                 (C.c_uint64 * max(1, ns))(*[int(v) for v in pend]), _fptr(sp))
        if rc < 0:
            _raise(rc)
    return buf


def pack_pad(rec, rows):
    """psdc_pack_pad: `rec` as a record of `rows` channels (the added ones empty) -- equal blocks for a gather."""
    b = np.ascontiguousarray(np.frombuffer(rec, dtype=np.uint8))
    if b.size < 32:
        _raise(ERR_ARG)
    n, nc = (int(v) for v in np.frombuffer(b[8:16].tobytes(), np.uint32))  # header {magic, version, n, n_channels, ...}
    if rows == nc:
        return b
    out = np.empty(lib().psdc_readout_bytes(n, rows), dtype=np.uint8)
    rc = lib().psdc_pack_pad(b.ctypes.data_as(C.c_void_p), b.size, out.ctypes.data_as(C.c_void_p), out.size, rows)
    if rc < 0:
        _raise(rc)
    return out


def unpack_info(buf, channel=0):
    """(n, n_channels, n_stages of `channel`) of a packed read-out record (bytes-like / uint8 array)."""
    b = np.frombuffer(buf, dtype=np.uint8)
    n, nc, ns = C.c_uint32(), C.c_uint32(), C.c_uint32()
    rc = lib().psdc_unpack_info(b.ctypes.data_as(C.c_void_p), b.size, channel, C.byref(n), C.byref(nc), C.byref(ns))
    if rc < 0:
        _raise(rc)
    return n.value, nc.value, ns.value


def unpack_stitch(buf, channel=0, opts=MergeOpts()):
    """PsdCascade::psd of one channel of a packed read-out record: identical to psd() on the handle that packed it."""
    b = np.frombuffer(buf, dtype=np.uint8)
    n, _, ns = unpack_info(b, channel)
    out = np.empty(max(1, ns * (n // 2 + 1)), dtype=np.float32)
    br = (_CBreak * max(1, ns))()
    plen, nb = C.c_size_t(), C.c_size_t()
    rc = lib().psdc_unpack_stitch(b.ctypes.data_as(C.c_void_p), b.size, channel, int(opts.keep_overlap), opts.min_count,
                                  int(opts.keep_transition_band), _fptr(out), out.size, C.byref(plen), br, ns, C.byref(nb))
    if rc < 0:
        _raise(rc)
    return out[:plen.value].copy(), [Break._from_c(br[i]) for i in range(nb.value)]


def var_eval(phase_psd, frequencies, tau, x_exp=-2, sinx_exp=4, clip=3.4028234663852886e38, dc_cut=2):
    """Var::eval (src/var.rs:26-45) with VarBuilder defaults (src/var.rs:7-17)."""
    p = np.ascontiguousarray(phase_psd, dtype=np.float32)
    f = np.ascontiguousarray(frequencies, dtype=np.float32)
    return float(lib().psdc_var_eval(x_exp, sinx_exp, clip, dc_cut, _fptr(p), _fptr(f), p.size, tau))


def trace_plot(psd, frequencies, fs=1.0, integrate=False, integral_start=0.0, integral_end=float("inf"), plot=True):
    """Trace::plot (src/bin/psd.rs:125-157): (integrated rms over [integral_start, integral_end] Hz, plot points)."""
    p = np.ascontiguousarray(psd, dtype=np.float32)
    f = np.ascontiguousarray(frequencies, dtype=np.float32)
    assert p.size == f.size
    rms, npts = C.c_float(), C.c_size_t()
    xy = np.empty((max(1, p.size), 2), dtype=np.float64)
    rc = lib().psdc_trace_plot(_fptr(p), _fptr(f), p.size, fs, int(integrate), integral_start, integral_end,
                               C.byref(rms), xy.ctypes.data_as(C.POINTER(C.c_double)) if plot else None, p.size,
                               C.byref(npts))
    if rc < 0:
        _raise(rc)
    return rms.value, (xy[:npts.value].copy() if plot else None)


def hbf_dec8(x, device=0):
    """HbfDec8 block processing from zero state on the device (src/psd.rs:246-253)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.empty(x.size // 8, dtype=np.float32)
    rc = lib().psdc_hbf_dec8(device, _fptr(x), x.size, _fptr(y))
    if rc < 0:
        _raise(rc)
    return y


def fill_noise_device(ptr, length, seed, first_index=0, device=0):
    rc = lib().psdc_fill_noise_device(device, C.c_void_p(ptr), length, seed, first_index)
    if rc < 0:
        _raise(rc)


def noise_host(length, seed, first_index=0):
    """Host twin of psdc_fill_noise_device: (u - 0.5) * sqrt(12), u from SplitMix64 seeded with
    mix64(seed + GAMMA), outputs first_index, first_index + 1, ... (src/psd.rs:604-606)."""
    gamma = np.uint64(0x9E3779B97F4A7C15)

    def mix64(x):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))

    with np.errstate(over="ignore"):
        key = mix64(np.array([seed & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64) + gamma)[0]
        i = np.arange(length, dtype=np.uint64) + np.uint64((first_index + 1) & 0xFFFFFFFFFFFFFFFF)
        x = mix64(key + i * gamma)
    u = (x >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    return ((u - np.float32(0.5)) * np.float32(3.4641016151377544)).astype(np.float32)


# ---- feed side (src/source.rs, src/de): byte formats only -------------------

ADCDAC_TRACES = ("ADC0", "ADC1", "DAC0", "DAC1")  # src/de/data.rs:37-80


def make_adcdac_frames(traces_i16, batches, seq0=0):
    """Serialise four int16 traces into AdcDac frames (src/de/frame.rs:5-37, data.rs:13).

    traces_i16: array [4, n_samples] of the RAW wire words (the DAC words are
    offset-binary on the wire, src/de/data.rs:64).  n_samples must be a multiple
    of 8*batches.  Returns (bytes, frame_size)."""
    t = np.ascontiguousarray(traces_i16, dtype="<i2")
    assert t.shape[0] == 4 and t.shape[1] % (8 * batches) == 0 and 0 < batches < 256
    nf = t.shape[1] // (8 * batches)
    frame_size = 8 + 64 * batches
    out = np.zeros((nf, frame_size), dtype=np.uint8)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = 0x7B, 0x05, 1, batches
    seq = (seq0 + np.arange(nf, dtype=np.uint64) * batches).astype("<u4")
    out[:, 4:8] = seq.view(np.uint8).reshape(nf, 4)
    # payload: frame, batch, channel, 8 samples
    pay = t.reshape(4, nf, batches, 8).transpose(1, 2, 0, 3)
    out[:, 8:] = np.ascontiguousarray(pay).view(np.uint8).reshape(nf, 64 * batches)
    return out.tobytes(), frame_size
