"""The frame-header scanner behind every frames call (csrc/frame_scan.h: run_start, scan_piece) on the CPU.

tests/host/frame_scan_check drives it as the callers do -- run by run, piece by piece, Loss committed with each piece -- over
blobs written here, and every line it prints is compared with a literal frame-by-frame walk: Frame::from_bytes through the
oracle's frame_decode (src/de/frame.rs:25-60, the payloads' size checks of src/de/data.rs), Loss::update as src/loss.rs:11-26
states it, stop at the first frame that fails.  Integers and strings only: no tolerance."""
import os
import random
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
OK, HEADER, FORMAT, SIZE = 0, -5, -6, -7          # PSDC_OK, PSDC_ERR_FRAME_HEADER / _FORMAT / _SIZE (include/psdcascade.h)
CODE = {0: OK, -1: HEADER, -2: FORMAT, -3: SIZE, -4: SIZE}  # frame_decode's status -> the ABI's code
BATCH_BYTES = {1: 64, 2: 56, 3: 80, 4: 24}        # src/de/data.rs:13, 86, 144, 168
MAGIC = b"\x7b\x05"


def frame(fmt, batches, seq, payload, magic=MAGIC):
    """one frame: header {magic, format id, batches, seq} (src/de/frame.rs:5-9) and `payload` bytes"""
    return magic + bytes([fmt, batches & 0xFF]) + struct.pack("<I", seq & 0xFFFFFFFF) + bytes((seq + i) & 0xFF for i in range(payload))


def run_of(fmt, count, payload, seq=0, gap=0):
    """`count` good frames of one format, seq continuing (plus `gap` batches between frames); returns (frames, next seq)"""
    b = payload // BATCH_BYTES[fmt]
    out = []
    for _ in range(count):
        out.append(frame(fmt, b, seq, payload))
        seq += b + gap
    return out, seq


def walk(ora, frames, adcdac_only):
    """the reference's per-frame `?` loop: the line frame_scan_check must print"""
    rc, good, received, dropped, next_seq, have_seq, runs = OK, 0, 0, 0, 0, 0, []
    for fr in frames:
        st, fmt, seq, bat, _ = ora.frame_decode(fr)
        if adcdac_only and fmt not in (0, 1):
            # psdc_process_adcdac_frames: any other format is UnknownFormat's code -- at Header::parse, where the id is looked at,
            # so before the payload's size is (frame_decode names the format of every frame whose header parses)
            st = -2
        if st != 0:
            rc = CODE[st]
            break
        received += bat
        if have_seq:
            dropped += (seq - next_seq) & 0xFFFFFFFF  # wrapping_sub
        next_seq = (seq + bat) & 0xFFFFFFFF           # wrapping_add
        have_seq = 1
        good += 1
        if runs and runs[-1][0] == fmt:
            runs[-1][1] += 1
        else:
            runs.append([fmt, 1])
    return " ".join([f"{rc} {good} {received} {dropped} {next_seq} {have_seq}"] + [f"{f}:{c}" for f, c in runs])


def blob(frames, piece, adcdac_only, frame_size=None):
    fs = len(frames[0]) if frame_size is None else frame_size
    assert all(len(f) == fs for f in frames)
    return struct.pack("<4Q", fs, len(frames), piece, 1 if adcdac_only else 0) + b"".join(frames)


def scan(tmp_path, blobs):
    """frame_scan_check over the blobs, headers in place and gathered: two lists of lines"""
    subprocess.run(["make", "-C", HOST, "frame_scan_check"], check=True, stdout=subprocess.DEVNULL)
    path = os.path.join(str(tmp_path), "blobs.bin")
    with open(path, "wb") as f:
        f.write(b"".join(blobs))
    out = []
    for view in ([], ["gathered"]):
        r = subprocess.run([os.path.join(HOST, "frame_scan_check"), path] + view, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out.append(r.stdout.splitlines())
    return out


def check(ora, tmp_path, cases):
    """cases: (name, frames, adcdac_only, frame_size or None).  Every case is scanned with piece limits 1, 2, 3, 7 and more than
    n_frames, through both views; every line must be the walk's."""
    blobs, want = [], []
    for name, frames, adc, fs in cases:
        line = walk(ora, frames, adc) if frames else "0 0 0 0 0 0"
        for piece in (1, 2, 3, 7, len(frames) + 5):
            blobs.append(blob(frames, piece, adc, fs) if frames else struct.pack("<4Q", fs or 72, 0, piece, int(adc)))
            want.append((f"{name}, pieces of {piece}", line))
    plain, gathered = scan(tmp_path, blobs)
    assert len(plain) == len(gathered) == len(want)
    for (name, line), a, b in zip(want, plain, gathered):
        assert a == line, f"{name}: got '{a}', the walk says '{line}'"
        assert b == line, f"{name} (gathered headers): got '{b}', the walk says '{line}'"
    return dict((name, line) for name, line in want)


def with_frame(frames, k, **change):
    """frames with frame k's header changed: magic=, fmt=, batches="""
    out = list(frames)
    f = bytearray(out[k])
    if "magic" in change:
        f[0:2] = change["magic"]
    if "fmt" in change:
        f[2] = change["fmt"]
    if "batches" in change:
        f[3] = change["batches"]
    out[k] = bytes(f)
    return out


def named_cases():
    """(name, frames, adcdac_only, frame_size, (rc, frames accepted) as the case is MEANT: checked against the walk)"""
    cases = []

    def add(name, frames, want, adc=False, fs=None):
        cases.append((name, frames, adc, fs, want))

    for fmt, bb in BATCH_BYTES.items():  # every format, alone: with and without seq gaps
        add(f"format {fmt}", run_of(fmt, 9, 3 * bb, seq=100)[0], (OK, 9))
        add(f"format {fmt} with gaps", run_of(fmt, 9, 2 * bb, seq=7, gap=5)[0], (OK, 9))
        add(f"format {fmt} header-only frames", run_of(fmt, 6, 0, seq=3, gap=2)[0], (OK, 6))
        add(f"format {fmt} seq wraps through 2^32", run_of(fmt, 8, 4 * bb, seq=2**32 - 10, gap=1)[0], (OK, 8))
        add(f"format {fmt} first seq 0xffffffff", run_of(fmt, 3, bb, seq=2**32 - 1)[0], (OK, 3))
        add(f"format {fmt} seq runs backwards", run_of(fmt, 2, bb, seq=50)[0] + run_of(fmt, 2, bb, seq=10)[0], (OK, 4))
        add(f"format {fmt} payload not a multiple of the batch", [frame(fmt, 1, 0, bb + 8)] * 3, (SIZE, 0))
        good = run_of(fmt, 7, 2 * bb)[0]
        add(f"format {fmt} hdr[3] one too many in frame 4", with_frame(good, 4, batches=3), (SIZE, 4))
        add(f"format {fmt} hdr[3] zero in frame 0", with_frame(good, 0, batches=0), (SIZE, 0))
        add(f"format {fmt} header-only frame that names a batch", with_frame(run_of(fmt, 4, 0)[0], 2, batches=1), (SIZE, 2))
        for k, where in ((0, "first"), (3, "a middle"), (6, "the last")):
            add(f"format {fmt} bad magic byte 0 on {where} frame", with_frame(good, k, magic=b"\x7a\x05"), (HEADER, k))
            add(f"format {fmt} bad magic byte 1 on {where} frame", with_frame(good, k, magic=b"\x7b\x04"), (HEADER, k))
        for bad_id in (0, 5, 255):
            add(f"format {fmt} unknown id {bad_id} at the run start", with_frame(good, 0, fmt=bad_id), (FORMAT, 0))
            add(f"format {fmt} unknown id {bad_id} in mid-run", with_frame(good, 5, fmt=bad_id), (FORMAT, 5))
        # doubly bad frames: the first check that fails names the error
        add(f"format {fmt} bad magic and unknown id", with_frame(good, 2, magic=b"\x00\x00", fmt=9), (HEADER, 2))
        add(f"format {fmt} unknown id and wrong hdr[3]", with_frame(good, 2, fmt=0, batches=9), (FORMAT, 2))
        add(f"format {fmt} bad magic and wrong hdr[3]", with_frame(good, 6, magic=b"\x7b\x00", batches=9), (HEADER, 6))
    # runs of several formats in one call: payloads that are whole batches of each (192 = 3 x 64 = 8 x 24, ...)
    for payload, fmts in ((192, (1, 4)), (168, (2, 4)), (240, (3, 4)), (448, (1, 2)), (320, (1, 3)), (560, (2, 3)), (1344, (1, 2, 4)),
                          (960, (1, 3, 4)), (1680, (2, 3, 4)), (2240, (1, 2, 3)), (0, (1, 2, 3, 4))):
        frames, seq = [], 2**32 - 40
        for i, fmt in enumerate(fmts + fmts[::-1] + fmts[:1]):
            fr, seq = run_of(fmt, 1 + (3 * i + payload) % 4, payload, seq=seq, gap=i % 2)
            frames += fr
        n = len(frames)
        add(f"runs of formats {fmts}, payload {payload}", frames, (OK, n))
        first_other = next(k for k, f in enumerate(frames) if f[2] != frames[0][2])
        add(f"runs of formats {fmts}, payload {payload}, bad magic at the second run's start",
            with_frame(frames, first_other, magic=b"\x05\x7b"), (HEADER, first_other))
        add(f"runs of formats {fmts}, payload {payload}, unknown id in the last frame", with_frame(frames, n - 1, fmt=5), (FORMAT, n - 1))
        add(f"runs of formats {fmts}, payload {payload}, wrong hdr[3] in the last frame",
            with_frame(frames, n - 1, batches=frames[n - 1][3] + 1), (SIZE, n - 1))
        if payload:
            # a format the payload is no whole number of batches of, in mid-call: a run starts there and takes nothing
            odd = next(f for f in (1, 2, 3, 4) if payload % BATCH_BYTES[f])
            add(f"runs of formats {fmts}, payload {payload}, a frame of format {odd} whose batches do not fit",
                with_frame(frames, n - 2, fmt=odd), (SIZE, n - 2))
        if fmts[0] == 1:  # the AdcDac-only rule: the run of AdcDac frames is taken, the next valid format is an error
            add(f"AdcDac only: formats {fmts}, payload {payload}", frames, (FORMAT, first_other), adc=True)
    # the AdcDac-only rule with a valid frame of another format first / in mid-run / unknown ids all the same
    adc = run_of(1, 8, 128, seq=11)[0]
    add("AdcDac only: all AdcDac", adc, (OK, 8), adc=True)
    for other, payload in ((2, 448), (3, 320), (4, 192)):
        a = run_of(1, 6, payload, seq=2**32 - 3)[0]
        o = run_of(other, 1, payload)[0]
        add(f"AdcDac only: a valid format {other} frame first", o + a, (FORMAT, 0), adc=True)
        add(f"AdcDac only: a valid format {other} frame in mid-run", a[:4] + o + a[4:], (FORMAT, 4), adc=True)
        add(f"not AdcDac only: the same frames", a[:4] + o + a[4:], (OK, 7))
    add("AdcDac only: unknown id in mid-run", with_frame(adc, 3, fmt=0), (FORMAT, 3), adc=True)
    add("AdcDac only: bad magic", with_frame(adc, 7, magic=b"\x00\x05"), (HEADER, 7), adc=True)
    add("AdcDac only: wrong hdr[3]", with_frame(adc, 1, batches=1), (SIZE, 1), adc=True)
    add("AdcDac only: header-only frames", run_of(1, 5, 0, seq=9, gap=1)[0], (OK, 5), adc=True)
    # the call's own checks
    add("no frames", [], (OK, 0))
    add("frames shorter than their header", [MAGIC + b"\x01\x00\x00"] * 3, (SIZE, 0), fs=5)
    add("one frame", run_of(4, 1, 24 * 255, seq=1)[0], (OK, 1))
    add("255 batches a frame, a gap of 2^32 - 255 (seq stands still)", [frame(4, 255, 77, 24 * 255)] * 4, (OK, 4))
    return cases


def random_case(rng):
    """a seeded blob and what it is MEANT to give: (frames, adcdac_only, rc, frames accepted)"""
    payload = rng.choice([0, 0, 24, 64, 56, 80, 192, 168, 240, 448, 320, 560, 1344, 960, 1680, 2240, 100, 8])
    fits = [f for f, bb in BATCH_BYTES.items() if payload % bb == 0 and payload // bb <= 255]
    adc = rng.random() < 0.25
    n = rng.choice([1, 2, 3, 5, 8, 13, 21, 40])
    seq = rng.choice([0, 1, 2**31, 2**32 - 1, 2**32 - rng.randrange(1, 600), rng.randrange(2**32)])
    frames, meant = [], []  # per frame: OK or the code it must stop the call with
    fmt = None
    while len(frames) < n:
        if adc and rng.random() < 0.8:
            fmt = 1
        elif fmt is None or rng.random() < 0.6:
            fmt = rng.choice(fits) if fits and rng.random() < 0.9 else rng.randrange(1, 5)
        for _ in range(min(n - len(frames), rng.randrange(1, 9))):
            ok = payload % BATCH_BYTES[fmt] == 0 and payload // BATCH_BYTES[fmt] <= 255
            b = payload // BATCH_BYTES[fmt] if ok else rng.randrange(256)
            if not ok and payload % BATCH_BYTES[fmt] == 0:
                b = (payload // BATCH_BYTES[fmt]) & 0xFF  # more than 255 batches: no header can say so
            f, code = frame(fmt, b, seq, payload), OK if ok else SIZE
            if adc and fmt != 1:
                code = FORMAT
            fault = rng.random()
            if fault < 0.02:
                f, code = with_frame([f], 0, magic=rng.choice([b"\x7b\x00", b"\x00\x05", b"\x05\x7b", b"\xff\xff"]))[0], HEADER
                if rng.random() < 0.5:
                    f = with_frame([f], 0, fmt=rng.choice([0, 5, 200]), batches=rng.randrange(256))[0]
            elif fault < 0.04:
                f, code = with_frame([f], 0, fmt=rng.choice([0, 5, 6, 128, 255]))[0], FORMAT
                if rng.random() < 0.5:
                    f = with_frame([f], 0, batches=rng.randrange(256))[0]
            elif fault < 0.06 and code == OK:
                f, code = with_frame([f], 0, batches=(b + rng.randrange(1, 256)) & 0xFF)[0], SIZE
            frames.append(f)
            meant.append(code)
            seq += b + (rng.choice([1, 7, 2**31, 2**32 - 2]) if rng.random() < 0.15 else 0)
    bad = next((k for k, c in enumerate(meant) if c != OK), None)
    return frames, adc, (OK if bad is None else meant[bad]), (n if bad is None else bad)


def meant(line):
    rc, good = line.split()[:2]
    return int(rc), int(good)


def test_named_cases(ora, tmp_path):
    cases = named_cases()
    assert len(cases) > 150
    for name, frames, adc, fs, want in cases:  # the cases are what they are meant to be, by the oracle's per-frame status
        if frames:
            assert meant(walk(ora, frames, adc)) == want, name
    lines = check(ora, tmp_path, [c[:4] for c in cases])
    # a few lines in full, by hand: Loss over a gap, over the wrap, and the runs
    assert lines["format 1 with gaps, pieces of 1"] == "0 9 18 40 65 1 1:9"            # 9 frames of 2 batches from seq 7, 8 gaps of 5
    assert lines["format 4 seq wraps through 2^32, pieces of 2"] == "0 8 32 7 29 1 4:8"  # 2^32 - 10 + 8 * 4 + 7 * 1 - 2^32
    assert lines["format 2 seq runs backwards, pieces of 7"] == f"0 4 4 {2**32 - 42} 12 1 2:4"  # 10 - 52, wrapping
    assert lines["AdcDac only: a valid format 4 frame in mid-run, pieces of 3"] == "-6 4 12 0 9 1 1:4"
    assert lines["not AdcDac only: the same frames, pieces of 3"] == f"0 7 26 {2**32 - 8} 15 1 1:4 4:1 1:2"  # 0 - 9 wrapping, then 9 - 8
    assert lines["frames shorter than their header, pieces of 1"] == "-7 0 0 0 0 0"


@pytest.mark.parametrize("seed", range(4))
def test_random_blobs(ora, tmp_path, seed):
    rng = random.Random(0x5EED0 + seed)
    cases, stops = [], set()
    for i in range(150):
        frames, adc, rc, good = random_case(rng)
        assert meant(walk(ora, frames, adc)) == (rc, good), f"seed {seed} blob {i}"  # the generator makes what it means to make
        cases.append((f"seed {seed} blob {i}", frames, adc, None))
        stops.add(rc)
    assert stops == {OK, HEADER, FORMAT, SIZE}
    check(ora, tmp_path, cases)
