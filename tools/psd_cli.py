#!/usr/bin/env python3
"""The receiver loop of the reference's `psd` binary (src/bin/psd.rs:158-221) without its GUI: a file-backed `Source` feeds one
`PsdCascade<512>` per trace (`:174-182`), and when the source is exhausted every trace is read out as `Cmd::Send` does (`:191-216`):
`psd(&merge_opts)`, `Break::frequencies`, `Trace::plot` (integrated RMS and plot points, `:125-157`).  Same option names and defaults
as `SourceOpts` (file-backed subset, src/source.rs:16-48) and `AcqOpts` (src/bin/psd.rs:31-72).
usage: tools/psd_cli.py (--file FRAMES [--frame-size N] | --raw RAW) [AcqOpts ...] [--max-bytes B] [--csv DIR]
Prints one line per trace: name, stages, averages of the top stage, bins, integrated RMS; --csv writes DIR/<trace>.csv (the plot points).
--pair X:Y (repeatable; trace labels or indices, frames only) also feeds the frames to a CsdCascadeBank(512, ...) and prints, per
pair, its bins and median coherence; with --csv it writes DIR/<x>__<y>.csv (f, |H1|, arg H1, coherence; H1 = Sxy / Sxx).
--zoom F0[:TRACE] (repeatable; F0 in cycles per sample, TRACE a label or index, default the first trace) also feeds that trace to a
ZoomCascade(512) around the carrier F0 and prints, or with --csv writes to DIR/zoom_<trace>_<F0>.csv, the lines offset,upper,lower
(the offset from the carrier in units of fs; upper / lower the density at F0 + offset / F0 - offset).
--zoom-pair F0:X:Y (repeatable; X, Y trace labels or indices) feeds the traces X and Y to a ZoomCsdCascade(512) with the carrier F0 on
both sides and prints, or with --csv writes to DIR/zoompair_<x>__<y>_<F0>.csv, the lines
offset,Saa,Sbb,Re Sab,Im Sab (at F0 + offset),Saa,Sbb,Re Sab,Im Sab (at F0 - offset); Sab = conj(Z_a) Z_b.
--iq I:Q[:F0] (repeatable) feeds a complex stream I + i Q to an IqCascade(512), retuned by F0 (cycles per sample, default 0: as it
is).  With --file, I and Q are traces of the frames (labels or indices, e.g. BI:BQ); without it they are two raw f32 files of equal
length (the planar pair; no --file / --raw is needed then).  Prints, or with --csv writes to DIR/iq_<i>__<q>_<F0>.csv, the lines
offset,upper,lower (the density of z at F0 + offset / F0 - offset; half of it is the two-sided density).
--iq-pair IA:QA:IB:QB[:F0] (repeatable) feeds the two complex streams IA + i QA and IB + i QB to an IqCsdCascade(512), both retuned by
the one carrier F0 (default 0).  Traces of the frames with --file, four raw f32 files of equal length without it, as for --iq.
Prints, or with --csv writes to DIR/iqpair_<ia>__<qa>__<ib>__<qb>_<F0>.csv, the lines of --zoom-pair:
offset,Saa,Sbb,Re Sab,Im Sab (at F0 + offset),Saa,Sbb,Re Sab,Im Sab (at F0 - offset); Sab = conj(Z_a) Z_b.
--sk [TRACE] (repeatable; TRACE a label or index, default the first trace; with --raw the file) also feeds that trace to an
SkCascade(512) and prints, or with --csv writes to DIR/sk_<trace>.csv, the lines frequency,psd,sk: the spectral kurtosis of every
bin beside its density (1: stationary Gaussian noise; 0: a line of constant amplitude; above 1: power that comes and goes; NaN
below two averages).  The summary line counts the bins more than 8 sk_sigma(count) away from 1.
--zoom-sk F0[:TRACE] (repeatable; as --zoom) feeds that trace to a ZoomSkCascade(512) around the carrier F0, and --iq-sk I:Q[:F0]
(repeatable; as --iq: traces of the frames with --file, two raw f32 files without it) the complex stream I + i Q to an
IqSkCascade(512).  Each prints, or with --csv writes to DIR/zoomsk_<trace>_<F0>.csv / DIR/iqsk_<i>__<q>_<F0>.csv, the lines
offset,psd,sk over the offsets -0.5 fs ... 0.5 fs from the carrier in ascending order (two_sided): the spectral kurtosis of the
sideband power beside its density.  Circular Gaussian noise reads 1 at every offset, 0 included; a real stream rises towards 2
where its own DC and Nyquist fall (offsets -F0 and 0.5 - F0).  The summary line counts the bins more than 8 sk_sigma(count) from 1.
--waterfall BLOCK:DEPTH[:TRACE] (repeatable; TRACE as for --sk) feeds that trace to a WaterfallCascade(512, block=BLOCK, depth=DEPTH),
and --zoom-waterfall F0:BLOCK:DEPTH[:TRACE] to a ZoomWaterfallCascade(512) around the carrier F0: per stage the newest DEPTH blocks
of BLOCK segments, each with its own PSD and spectral kurtosis (every segment has weight 1: --avg and --avg-max do not apply).
Each prints, or with --csv writes to DIR/waterfall_<trace>_stage<k>.csv / DIR/zoom_waterfall_<trace>_<F0>_stage<k>.csv, one file a
stage: a header line with the block indices and counts, then one line a block, oldest first, with the PSD of every bin followed by
the SK of every bin (the zoom option: upper then lower sideband of each).
--bank-readout reads the spectra and frequencies of all traces of the main bank with ONE call (bankread.bank_psd: every trace
stitched on the device in one launch, one copy to the host) where the default asks psd() trace by trace; the lines and the files
are the same, byte for byte.  With --pair it also reads the rows and frequencies of all pairs with ONE call (crossread.bank_csd)
where the default asks csd() pair by pair; coherence and H1 are formed from those rows as before, so the lines and files are the same.
--var KIND[:PER_DECADE] (repeatable, at most 4; KIND one of avar, mvar, fvar; needs --bank-readout) prints behind the traces the
Allan, modified Allan or main-lobe deviation curve of every trace of the main bank, all from ONE call (bankvar.bank_var: one launch
reads the accumulators, no spectrum is copied): a header line a trace and kind, then one line `tau,deviation` a tau, with --csv in
DIR/<trace>_<kind>.csv.  The spectra are taken as phase PSDs; taus run from one sample to the period of the lowest bin that counts, with
PER_DECADE points a decade (default 10, the largest given; at most 4096 taus), printed in seconds (tau / fs) with fs sqrt(var).
--robust KIND[:NSIGMA] (repeatable; KIND one of median, min, max, excised) adds to every --waterfall / --zoom-waterfall trace the
robust read-out of every stage (robust.stage_robust: over the stage's complete blocks, made on the device): behind the lines above,
or with --csv in DIR/<the stage's file name>_robust.csv, a header line with the rows and blocks considered, then one line a KIND
with the value of every bin (the zoom option: upper then lower).  excised is the mean of the blocks whose spectral kurtosis lies
within NSIGMA (default 3) sk_sigma(BLOCK) of 1, and is followed by a line with the number of blocks kept a bin.
--zoom-ampm F0[:TRACE] (repeatable; as --zoom) feeds that trace to a ZoomAmPmCascade(512) around the carrier F0, and --iq-ampm
I:Q[:F0] (repeatable; as --iq) the complex stream I + i Q to an IqAmPmCascade(512).  Both run without a detrend whatever --detrend
says: the carrier's amplitude and phase are read from bin 0 (carrier()), which a detrend removes.  Each prints, or with --csv writes
to DIR/zoomampm_<trace>_<F0>.csv / DIR/iqampm_<i>__<q>_<F0>.csv, the lines offset,S_am,S_pm,Re S_ampm,Im S_ampm: the amplitude
noise, phase noise and AM-PM cross spectra of the carrier (am_pm(): relative to the carrier, a linear small-modulation split).  The
summary line gives the carrier's power, angle and lock (1: the carrier sits at F0; towards 0: it turned during the average and the
split means nothing).
--zoom-ampm-pair F0:X:Y (repeatable; as --zoom-pair) feeds the traces X and Y to a ZoomAmPmCsdCascade(512) with the carrier F0 on both
sides, and --iq-ampm-pair IA:QA:IB:QB[:F0] (repeatable; as --iq-pair) two complex streams to an IqAmPmCsdCascade(512); no detrend,
as for --zoom-ampm.  Each prints, or with --csv writes to DIR/zoomampmpair_<x>__<y>_<F0>.csv /
DIR/iqampmpair_<ia>__<qa>__<ib>__<qb>_<F0>.csv, the lines offset, then Re and Im of s_am, s_pm, s_am_pm, s_pm_am: the cross spectra
of the two channels' amplitude and phase modulation (am_pm_cross(): what both channels share stays, each channel's own noise
averages down).  The summary line gives p_ab = |A_a| |A_b|, the angles of w = conj(v_a) v_b and q = v_a v_b, and the two locks.
--sample-format s16|s8 (default f32: everything above, unchanged) reads raw INTEGER files and feeds them as they are through the
integer feeds (process_int; the device converts, sample = integer * --scale, default 2^-15 for s16 and 2^-7 for s8).  The options
then name files, and no --file / --raw is read: --zoom F0:FILE and --zoom-pair F0:FILEA:FILEB take files of real integers, --iq
FILE[:F0] and --iq-pair FILEA:FILEB[:F0] files of interleaved (re, im) integer pairs (sc16 / sc8, an SDR's native output); --raw
FILE is the plain spectrum of a file of real integers (PsdCascade.process_int) and --pair FILEX:FILEY the cross spectrum of two
such files (CsdCascade.process_int).  --file (frames) is refused.  The printed lines and the --csv files are those of the f32
options."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def var_curves(pkg, a, bank, merge, names):
    """--var: the deviation curves of every trace of the main bank from one bankvar.bank_var call"""
    from stabilizer_stream_amd import bankread, bankvar
    kinds, per_decade = [], 0
    for spec in a.var:
        kind, _, n = spec.partition(":")
        if kind not in ("avar", "mvar", "fvar") or (n and not n.isdigit()) or (n and int(n) < 1):
            raise SystemExit(f"--var {spec}: KIND[:PER_DECADE] with KIND one of avar, mvar, fvar")
        kinds.append(kind)
        per_decade = max(per_decade, int(n) if n else 0)
    if len(kinds) > bankvar.MAX_VARS:
        raise SystemExit(f"--var: at most {bankvar.MAX_VARS} curves a call")
    vs = [getattr(bankvar.Var, k)() for k in kinds]
    lay = bankread.layout(bank, None, merge)
    lowest = [pkg.Break.frequencies(br)[vs[0].dc_cut] for ln, br in zip(lay["lens"], lay["breaks"]) if ln > vs[0].dc_cut]
    if not lowest:
        print("var: no samples")
        return
    decades = max(0.0, float(np.log10(1.0 / min(lowest))))
    count = min(bankvar.MAX_TAUS, int(decades * (per_decade or 10)) + 1)
    taus = np.logspace(0.0, decades, count).astype(np.float32)
    r = bankvar.bank_var(bank, taus, vs, None, merge)  # float64 [traces][kinds][taus]
    for i, name in enumerate(names):
        if r["lens"][i] == 0:
            continue
        for k, kind in enumerate(kinds):
            dev = a.fs * np.sqrt(r["var"][i, k])
            print(f"{name}: {kind} taus {count} bins {r['lens'][i]}")
            lines = [f"{t / a.fs:.9g},{d:.9g}\n" for t, d in zip(taus, dev)]
            if a.csv:
                safe = "".join(ch if ch.isalnum() else "_" for ch in name)
                with open(os.path.join(a.csv, f"{safe}_{kind}.csv"), "w") as f:
                    f.writelines(lines)
            else:
                sys.stdout.writelines(lines)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-f", "--file")
    ap.add_argument("--frame-size", type=int, default=8 + 30 * 2 * 6 * 4)   # src/source.rs:31
    ap.add_argument("--repeat", action="store_true")
    ap.add_argument("-r", "--raw")
    ap.add_argument("-d", "--detrend", default="mean", choices=["none", "midpoint", "span", "mean"])  # src/bin/psd.rs:34-35
    ap.add_argument("--fs", type=float, default=1.0)
    ap.add_argument("--avg-max", type=int, default=1000)
    ap.add_argument("--avg-min", type=int, default=1)
    ap.add_argument("-a", "--avg", type=int, default=0xFFFFFFFF)
    ap.add_argument("--keep-overlap", action="store_true")
    ap.add_argument("--keep-transition-band", action="store_true")
    ap.add_argument("--integrate", action="store_true")
    ap.add_argument("--integral-start", type=float, default=1e-6)
    ap.add_argument("--integral-end", type=float, default=0.5)
    ap.add_argument("--max-bytes", type=int, default=None, help="stop after this many input bytes (needed with --repeat)")
    ap.add_argument("--csv", default=None, help="directory for the plot points of every trace")
    ap.add_argument("--pair", action="append", default=[], help="X:Y -- cross spectrum of traces X and Y (repeatable)")
    ap.add_argument("--zoom", action="append", default=[], help="F0[:TRACE] -- two-sided spectrum around the carrier F0 (repeatable)")
    ap.add_argument("--zoom-pair", action="append", default=[],
                    help="F0:X:Y -- two-sided auto and cross spectra of traces X and Y around the carrier F0 (repeatable)")
    ap.add_argument("--iq", action="append", default=[],
                    help="I:Q[:F0] -- two-sided spectrum of the complex stream I + i Q, retuned by F0 (repeatable)")
    ap.add_argument("--iq-pair", action="append", default=[],
                    help="IA:QA:IB:QB[:F0] -- two-sided auto and cross spectra of two complex streams, retuned by F0 (repeatable)")
    ap.add_argument("--sk", action="append", nargs="?", const="", default=[],
                    help="[TRACE] -- spectral kurtosis of every bin beside the PSD of that trace (repeatable; default the first trace)")
    ap.add_argument("--zoom-sk", action="append", default=[],
                    help="F0[:TRACE] -- two-sided spectral kurtosis beside the spectrum around the carrier F0 (repeatable)")
    ap.add_argument("--iq-sk", action="append", default=[],
                    help="I:Q[:F0] -- two-sided spectral kurtosis beside the spectrum of the complex stream I + i Q (repeatable)")
    ap.add_argument("--waterfall", action="append", default=[],
                    help="BLOCK:DEPTH[:TRACE] -- PSD and spectral kurtosis of that trace against time: per stage the newest DEPTH blocks of "
                         "BLOCK segments (repeatable)")
    ap.add_argument("--zoom-waterfall", action="append", default=[],
                    help="F0:BLOCK:DEPTH[:TRACE] -- the same, two-sided around the carrier F0 (repeatable)")
    ap.add_argument("--bank-readout", action="store_true",
                    help="read every trace's spectrum and frequencies with ONE bankread.bank_psd call, and every --pair's rows with ONE "
                         "crossread.bank_csd call (the same output, byte for byte)")
    ap.add_argument("--var", action="append", default=[],
                    help="KIND[:PER_DECADE] -- with --bank-readout: the avar, mvar or fvar deviation curve of every trace from one "
                         "bankvar.bank_var call (repeatable, at most 4)")
    ap.add_argument("--robust", action="append", default=[],
                    help="KIND[:NSIGMA] -- with --waterfall / --zoom-waterfall: per stage the median, min, max or SK-excised mean (within "
                         "NSIGMA sk_sigma of 1, default 3) over its complete blocks (repeatable)")
    ap.add_argument("--zoom-ampm", action="append", default=[],
                    help="F0[:TRACE] -- amplitude and phase noise spectra of the carrier F0 of that trace (repeatable)")
    ap.add_argument("--iq-ampm", action="append", default=[],
                    help="I:Q[:F0] -- amplitude and phase noise spectra of the carrier of the complex stream I + i Q (repeatable)")
    ap.add_argument("--zoom-ampm-pair", action="append", default=[],
                    help="F0:X:Y -- cross spectra of the amplitude and phase modulation of traces X and Y on the carrier F0 (repeatable)")
    ap.add_argument("--iq-ampm-pair", action="append", default=[],
                    help="IA:QA:IB:QB[:F0] -- cross spectra of the amplitude and phase modulation of two complex streams (repeatable)")
    ap.add_argument("--sample-format", default="f32", choices=["f32", "s16", "s8"],
                    help="s16 / s8: --raw, --pair, --zoom, --zoom-pair, --iq and --iq-pair name raw integer files (real integers / interleaved pairs)")
    ap.add_argument("--scale", type=float, default=None, help="with --sample-format s16 / s8: sample = integer * SCALE (default 2^-15 / 2^-7)")
    a = ap.parse_args(argv)
    if a.sample_format != "f32":
        if a.file or not (a.raw or a.pair or a.zoom or a.zoom_pair or a.iq or a.iq_pair):
            raise SystemExit("--sample-format s16 / s8 takes --raw, --pair, --zoom, --zoom-pair, --iq or --iq-pair with raw integer files, "
                             "and no --file")
        import __graft_entry__ as entry
        return int_feeds(entry.load_package(), a)
    if a.scale is not None:
        raise SystemExit("--scale needs --sample-format s16 or s8")
    if a.pair and a.raw:
        raise SystemExit("--pair needs --file")
    if a.var and not a.bank_readout:
        raise SystemExit("--var needs --bank-readout")
    import __graft_entry__ as entry
    pkg = entry.load_package()
    from stabilizer_stream_amd import source
    if (a.iq or a.iq_pair or a.iq_sk or a.iq_ampm or a.iq_ampm_pair) and not a.file:  # the planar raw files: the only input these options need
        merge = pkg.MergeOpts(keep_overlap=a.keep_overlap, min_count=a.avg_min, keep_transition_band=a.keep_transition_band)
        if a.csv:
            os.makedirs(a.csv, exist_ok=True)
        if a.iq_sk:
            iq_sk_streams(pkg, source, a, merge, None)
        if a.iq_ampm:
            iq_ampm_streams(pkg, source, a, merge, None)
        if a.iq:
            iq_streams(pkg, source, a, merge, None)
        if a.iq_pair:
            iq_pairs(pkg, source, a, merge, None)
        if a.iq_ampm_pair:
            iq_ampm_pairs(pkg, source, a, merge, None)
        if not a.raw:
            return 0
    integral_start, integral_end = a.integral_start * a.fs, a.integral_end * a.fs  # src/bin/psd.rs:161-162
    src = source.Source(source.SourceOpts(file=a.file, frame_size=a.frame_size, repeat=a.repeat, raw=a.raw), pkg)
    if a.raw:
        names = ["raw"]
    else:  # the labels of Payload::traces for the file's format (its first frame's header, src/de/frame.rs:25-37)
        with open(a.file, "rb") as f:
            head = f.read(8)
        if len(head) < 8 or head[0] != 0x7B or head[1] != 0x05 or not 1 <= head[2] <= 4:
            raise SystemExit("source: Invalid frame header")
        names = list(pkg.TRACE_NAMES[pkg.Format(head[2])])
    bank = pkg.PsdCascadeBank(1 << 9, len(names))  # PsdCascade::<{ 1 << 9 }> (src/bin/psd.rs:176)
    bank.set_detrend(pkg.Detrend[a.detrend.upper()])
    bank.set_avg(pkg.AvgOpts(limit=max(0, a.avg_max - 1), count=max(0, a.avg - 1)))  # AcqOpts::avg_opts (:74-79)
    merge = pkg.MergeOpts(keep_overlap=a.keep_overlap, min_count=a.avg_min, keep_transition_band=a.keep_transition_band)  # :81-87
    total = 0
    while a.max_bytes is None or total < a.max_bytes:
        got = src.feed(bank, max_bytes=(64 << 20) if a.max_bytes is None else min(64 << 20, max(a.frame_size, a.max_bytes - total)))
        if got == 0:
            break
        total += got
    src.close()
    if a.csv:
        os.makedirs(a.csv, exist_ok=True)
    if a.bank_readout:  # every trace stitched on the device in one launch, one copy (include/psdcascade_readout.h)
        from stabilizer_stream_amd import bankread
        allrows = bankread.bank_psd(bank, None, merge, frequencies=True)
    for i, name in enumerate(names):
        if bank.num_stages(i) == 0:
            print(f"{name}: no samples")
            continue
        if a.bank_readout:
            ln, breaks = allrows["lens"][i], allrows["breaks"][i]
            psd, freqs = allrows["psd"][i, :ln], allrows["frequencies"][i, :ln]
        else:
            psd, breaks = bank.psd(i, merge)
            freqs = pkg.Break.frequencies(breaks)
        rms, xy = pkg.trace_plot(psd, freqs, fs=a.fs, integrate=a.integrate, integral_start=integral_start, integral_end=integral_end)
        top = bank.stage_info(i, 0)["count"]
        print(f"{name}: stages {bank.num_stages(i)} top-stage averages {top} bins {psd.size} breaks {len(breaks)} rms {rms:.9g}")
        if a.csv:
            safe = "".join(ch if ch.isalnum() else "_" for ch in name)
            with open(os.path.join(a.csv, safe + ".csv"), "w") as f:
                f.writelines(f"{x:.9g},{y:.9g}\n" for x, y in xy)
    if a.var:
        var_curves(pkg, a, bank, merge, names)
    if a.pair:
        cross_pairs(pkg, source, a, merge)
    if a.zoom:
        zoom_traces(pkg, source, a, merge, names)
    if a.zoom_pair:
        zoom_pairs(pkg, source, a, merge, names)
    if a.sk:
        sk_traces(pkg, source, a, merge, names)
    if a.zoom_sk:
        zoom_sk_traces(pkg, source, a, merge, names)
    if a.iq_sk and a.file:
        iq_sk_streams(pkg, source, a, merge, names)
    if a.waterfall:
        waterfall_traces(pkg, source, a, names)
    if a.zoom_waterfall:
        zoom_waterfall_traces(pkg, source, a, names)
    if a.zoom_ampm:
        zoom_ampm_traces(pkg, source, a, merge, names)
    if a.iq_ampm and a.file:
        iq_ampm_streams(pkg, source, a, merge, names)
    if a.iq and a.file:
        iq_streams(pkg, source, a, merge, names)
    if a.iq_pair and a.file:
        iq_pairs(pkg, source, a, merge, names)
    if a.zoom_ampm_pair:
        zoom_ampm_pairs(pkg, source, a, merge, names)
    if a.iq_ampm_pair and a.file:
        iq_ampm_pairs(pkg, source, a, merge, names)
    loss = bank.loss()
    if not a.raw:
        tot = loss["received"] + loss["dropped"]
        print(f"loss: {loss['dropped']} of {tot} batches ({(loss['dropped'] / tot if loss['received'] else 0.0):.3e})")  # Loss::analyze
    bank.close()
    return 0


def cross_pairs(pkg, source, a, merge):
    """--pair: the file's frames again, through the same Source reads, into one cross cascade per pair"""
    pairs = [tuple(p.split(":", 1)) for p in a.pair]
    if any(len(p) != 2 for p in pairs):
        raise SystemExit("--pair takes X:Y")
    pairs = [tuple(int(t) if t.isdigit() else t for t in p) for p in pairs]
    cross = pkg.CsdCascadeBank(1 << 9, len(pairs))
    cross.set_detrend(pkg.Detrend[a.detrend.upper()])
    cross.set_avg(pkg.AvgOpts(limit=max(0, a.avg_max - 1), count=max(0, a.avg - 1)))

    class Feed:  # what Source.feed calls on a bank
        def process_frames(self, buf, fs):
            cross.process_frames(buf, fs, pairs)

    src = source.Source(source.SourceOpts(file=a.file, frame_size=a.frame_size, repeat=a.repeat), pkg)
    total = 0
    while a.max_bytes is None or total < a.max_bytes:
        got = src.feed(Feed(), max_bytes=(64 << 20) if a.max_bytes is None else min(64 << 20, max(a.frame_size, a.max_bytes - total)))
        if got == 0:
            break
        total += got
    src.close()
    if a.bank_readout:  # every pair stitched on the device in one launch, one copy (include/psdcascade_crossread.h)
        from stabilizer_stream_amd import crossread
        allrows = crossread.bank_csd(cross, None, merge, frequencies=True)
    for i, (x, y) in enumerate(pairs):
        label = f"{x}:{y}"
        if cross.num_stages(i) == 0:
            print(f"{label}: no samples")
            continue
        if a.bank_readout:
            ln = allrows["lens"][i]
            sxx, syy, sxy = (allrows[k][i, :ln] for k in ("sxx", "syy", "sxy"))
            freqs = allrows["frequencies"][i, :ln] * a.fs
        else:
            sxx, syy, sxy, breaks = cross.csd(i, merge)
            freqs = pkg.Break.frequencies(breaks) * a.fs
        coh = pkg.coherence(sxx, syy, sxy)
        h1 = pkg.transfer(sxx, sxy)
        print(f"{label}: bins {sxx.size} median coherence {np.nanmedian(coh):.6g}")
        if a.csv:
            safe = "__".join("".join(ch if ch.isalnum() else "_" for ch in str(t)) for t in (x, y))
            with open(os.path.join(a.csv, safe + ".csv"), "w") as f:
                f.writelines(f"{fr:.9g},{abs(h):.9g},{np.angle(h):.9g},{c:.9g}\n" for fr, h, c in zip(freqs, h1, coh))
    cross.close()


def trace_arg(tr, names, opt):
    """a trace given as a label or an index ("" is the first trace)"""
    idx = 0 if tr == "" else int(tr) if tr.isdigit() else (names.index(tr) if tr in names else -1)
    if not 0 <= idx < len(names):
        raise SystemExit(f"{opt}: unknown trace {tr!r}")
    return idx


def host_traces(source, pkg, a, units, process):
    """The source once more through Source's host traces (raw files and frame files alike): unit i takes the traces units[i] (a
    tuple of indices) of every read; process(i, [samples of each]) is called about every 2^20 samples"""
    src = source.Source(source.SourceOpts(file=a.file, frame_size=a.frame_size, repeat=a.repeat, raw=a.raw), pkg)
    total, held, pend = 0, 0, [[[] for _ in u] for u in units]

    def flush():
        for i, chunks in enumerate(pend):
            if chunks[0]:
                process(i, [np.concatenate(c) for c in chunks])
                for c in chunks:
                    c.clear()

    while a.max_bytes is None or total < a.max_bytes:
        try:
            traces = src.get()  # [(label, samples)] of one frame, or one chunk of a raw file
        except EOFError:
            break
        if src.eof:
            break
        for i, u in enumerate(units):
            for c, idx in enumerate(u):
                pend[i][c].append(traces[idx][1])
        total += a.frame_size if a.file else traces[0][1].nbytes
        held += traces[0][1].size
        if held >= 1 << 20:
            flush()
            held = 0
    flush()
    src.close()


def zoom_traces(pkg, source, a, merge, names):
    """--zoom: the named trace of every read (host_traces) into one zoom cascade per carrier"""
    want = []
    for z in a.zoom:
        f0, _, tr = z.partition(":")
        want.append((float(f0), trace_arg(tr, names, "--zoom")))
    bank = pkg.ZoomCascadeBank(1 << 9, len(want))
    bank.set_detrend(pkg.Detrend[a.detrend.upper()])
    bank.set_avg(pkg.AvgOpts(limit=max(0, a.avg_max - 1), count=max(0, a.avg - 1)))
    used = [bank.set_carrier(i, f0=f0) for i, (f0, _) in enumerate(want)]
    host_traces(source, pkg, a, [(idx,) for _, idx in want], lambda i, xs: bank.process(i, xs[0]))
    for i, (_, idx) in enumerate(want):
        label = f"zoom {names[idx]} @ {used[i]:.12g}"
        if bank.num_stages(i) == 0:
            print(f"{label}: no samples")
            continue
        up, lo, breaks = bank.psd(i, merge)
        off = pkg.Break.frequencies(breaks) * a.fs
        print(f"{label}: stages {bank.num_stages(i)} bins {up.size} breaks {len(breaks)}")
        lines = [f"{o:.9g},{u:.9g},{w:.9g}\n" for o, u, w in zip(off, up, lo)]
        if a.csv:
            safe = "".join(ch if ch.isalnum() else "_" for ch in f"zoom_{names[idx]}_{used[i]:.9g}")
            with open(os.path.join(a.csv, safe + ".csv"), "w") as f:
                f.writelines(lines)
        else:
            sys.stdout.writelines(lines)
    bank.close()


def sk_traces(pkg, source, a, merge, names):
    """--sk: the named trace of every read (host_traces) into one spectral kurtosis cascade each"""
    want = [trace_arg(tr, names, "--sk") for tr in a.sk]
    bank = pkg.SkCascadeBank(1 << 9, len(want))
    bank.set_detrend(pkg.Detrend[a.detrend.upper()])
    bank.set_avg(pkg.AvgOpts(limit=max(0, a.avg_max - 1), count=max(0, a.avg - 1)))
    host_traces(source, pkg, a, [(idx,) for idx in want], lambda i, xs: bank.process(i, xs[0]))
    for i, idx in enumerate(want):
        label = f"sk {names[idx]}"
        if bank.num_stages(i) == 0:
            print(f"{label}: no samples")
            continue
        psd, breaks = bank.psd(i, merge)
        sk, _ = bank.sk(i, merge)
        freqs = pkg.Break.frequencies(breaks) * a.fs
        sigma = np.concatenate([np.full(b.bins.stop - b.bins.start, pkg.sk_sigma(max(b.count, 1))) for b in breaks if b.include] or [np.zeros(0)])
        with np.errstate(invalid="ignore"):
            odd = int(np.sum(np.abs(sk - 1.0) > 8.0 * sigma))
        print(f"{label}: stages {bank.num_stages(i)} bins {psd.size} breaks {len(breaks)} median sk {np.nanmedian(sk) if sk.size else float('nan'):.6g} "
              f"bins beyond 8 sigma of 1: {odd}")
        lines = [f"{fr:.9g},{p:.9g},{k:.9g}\n" for fr, p, k in zip(freqs, psd, sk)]
        if a.csv:
            safe = "".join(ch if ch.isalnum() else "_" for ch in f"sk_{names[idx]}")
            with open(os.path.join(a.csv, safe + ".csv"), "w") as f:
                f.writelines(lines)
        else:
            sys.stdout.writelines(lines)
    bank.close()


def waterfall_report(pkg, g, label, stem, a):
    """the read-out of a WaterfallCascade / ZoomWaterfallCascade: the summary line, and per stage the images of image(): one line a
    block, oldest first, the PSD of every bin followed by the SK of every bin (a zoom object: upper then lower of each), behind a
    header line with the block indices and counts"""
    ns = g.num_stages()
    if ns == 0:
        print(f"{label}: no samples")
        return
    print(f"{label}: {ns} stages, block {g.block} depth {g.depth}, rows " + " ".join(str(g.stage_blocks(k)["rows_valid"]) for k in range(ns)))
    for k in range(ns):
        psd, sk, idx, cnt = g.image(k)
        span = g.block_span(k, int(idx[-1])) if idx.size else range(0)
        head = (f"# stage {k}: blocks {' '.join(map(str, idx.tolist()))}; counts {' '.join(map(str, cnt.tolist()))}; columns: psd then sk, "
                f"{psd[0].size if idx.size else 0} each; the newest block nominally ends at input sample {span.stop}\n")
        lines = [",".join(f"{v:.9g}" for v in np.concatenate([p.ravel(), s.ravel()])) + "\n" for p, s in zip(psd, sk)]
        if a.csv:
            safe = "".join(ch if ch.isalnum() else "_" for ch in f"{stem}_stage{k}")
            with open(os.path.join(a.csv, safe + ".csv"), "w") as f:
                f.write(head)
                f.writelines(lines)
        else:
            sys.stdout.write(head)
            sys.stdout.writelines(lines)
        if a.robust:
            robust_report(g, k, stem, a)


def robust_spec(z):
    """KIND[:NSIGMA] of --robust: (kind, nsigma)"""
    kind, _, ns = z.partition(":")
    try:
        nsigma = float(ns) if ns else 3.0
    except ValueError:
        nsigma = -1.0
    if kind not in ("median", "min", "max", "excised") or not nsigma > 0 or (ns and kind != "excised"):
        raise SystemExit("--robust takes median, min, max or excised[:NSIGMA]")
    return kind, nsigma


def robust_report(g, k, stem, a):
    """--robust: the robust rows of stage k of a waterfall object, one line a KIND (excised: a line of kept counts behind it)"""
    from stabilizer_stream_amd import robust
    lines, rows = [], None
    for kind, nsigma in map(robust_spec, a.robust):
        r = robust.stage_robust(g, k, sk_limits=robust.sk_limits(g.block, nsigma) if kind == "excised" else None)
        rows = r
        lines.append(",".join(f"{v:.9g}" for v in r[kind].ravel()) + "\n")
        if kind == "excised":
            lines.append(",".join(str(int(v)) for v in r["kept"].ravel()) + "\n")
    blocks = f"blocks {rows['first_block']} ... {rows['last_block']}" if rows["rows"] else "no complete block"
    head = (f"# stage {k} robust: {rows['rows']} rows, {blocks}; lines: " +
            " ".join(z + (" kept" if z.startswith("excised") else "") for z in a.robust) + "\n")
    if a.csv:
        safe = "".join(ch if ch.isalnum() else "_" for ch in f"{stem}_stage{k}_robust")
        with open(os.path.join(a.csv, safe + ".csv"), "w") as f:
            f.write(head)
            f.writelines(lines)
    else:
        sys.stdout.write(head)
        sys.stdout.writelines(lines)


def waterfall_spec(z, opt, lead):
    """BLOCK:DEPTH[:TRACE] behind `lead` leading fields"""
    parts = z.split(":", lead + 2)
    if len(parts) < lead + 2 or not (parts[lead].isdigit() and parts[lead + 1].isdigit()):
        raise SystemExit(f"{opt} takes {'F0:' if lead else ''}BLOCK:DEPTH[:TRACE]")
    return parts[:lead], int(parts[lead]), int(parts[lead + 1]), parts[lead + 2] if len(parts) > lead + 2 else ""


def waterfall_traces(pkg, source, a, names):
    """--waterfall BLOCK:DEPTH[:TRACE]: the named trace of every read (host_traces) into one waterfall cascade each"""
    for z in a.waterfall:
        _, block, depth, tr = waterfall_spec(z, "--waterfall", 0)
        idx = trace_arg(tr, names, "--waterfall")
        g = pkg.WaterfallCascade(1 << 9, block=block, depth=depth)
        g.set_detrend(pkg.Detrend[a.detrend.upper()])
        host_traces(source, pkg, a, [(idx,)], lambda i, xs: g.process(xs[0]))
        waterfall_report(pkg, g, f"waterfall {names[idx]}", f"waterfall_{names[idx]}", a)
        g.close()


def zoom_waterfall_traces(pkg, source, a, names):
    """--zoom-waterfall F0:BLOCK:DEPTH[:TRACE]: the named trace into one zoom waterfall cascade around the carrier F0 each"""
    for z in a.zoom_waterfall:
        (f0,), block, depth, tr = waterfall_spec(z, "--zoom-waterfall", 1)
        idx = trace_arg(tr, names, "--zoom-waterfall")
        g = pkg.ZoomWaterfallCascade(1 << 9, f0=float(f0), block=block, depth=depth)
        g.set_detrend(pkg.Detrend[a.detrend.upper()])
        host_traces(source, pkg, a, [(idx,)], lambda i, xs: g.process(xs[0]))
        waterfall_report(pkg, g, f"zoom_waterfall {names[idx]} @ {g.f0:.12g}", f"zoom_waterfall_{names[idx]}_{g.f0:.9g}", a)
        g.close()


def two_sided_sk_report(pkg, bank, c, label, stem, a, merge):
    """the read-out of one channel of a ZoomSkCascadeBank / IqSkCascadeBank: the summary line, and offset,psd,sk in two_sided order"""
    if bank.num_stages(c) == 0:
        print(f"{label}: no samples")
        return
    up, lo, breaks = bank.psd(c, merge)
    sup, slo, _ = bank.sk(c, merge)
    off, psd = pkg.two_sided(up, lo, breaks)
    _, sk = pkg.two_sided(sup, slo, breaks)
    sig = np.concatenate([np.full(b.bins.stop - b.bins.start, pkg.sk_sigma(max(b.count, 1))) for b in breaks if b.include] or [np.zeros(0)])
    _, sigma = pkg.two_sided(sig, sig, breaks)
    with np.errstate(invalid="ignore"):
        odd = int(np.sum(np.abs(sk - 1.0) > 8.0 * sigma))
    print(f"{label}: stages {bank.num_stages(c)} bins {psd.size} breaks {len(breaks)} median sk {np.nanmedian(sk) if sk.size else float('nan'):.6g} "
          f"bins beyond 8 sigma of 1: {odd}")
    lines = [f"{o:.9g},{p:.9g},{k:.9g}\n" for o, p, k in zip(off * a.fs, psd, sk)]
    if a.csv:
        safe = "".join(ch if ch.isalnum() else "_" for ch in stem)
        with open(os.path.join(a.csv, safe + ".csv"), "w") as f:
            f.writelines(lines)
    else:
        sys.stdout.writelines(lines)


def zoom_sk_traces(pkg, source, a, merge, names):
    """--zoom-sk: the named trace of every read (host_traces) into one zoom spectral kurtosis cascade per carrier"""
    want = []
    for z in a.zoom_sk:
        f0, _, tr = z.partition(":")
        want.append((float(f0), trace_arg(tr, names, "--zoom-sk")))
    bank = pkg.ZoomSkCascadeBank(1 << 9, len(want))
    bank.set_detrend(pkg.Detrend[a.detrend.upper()])
    bank.set_avg(pkg.AvgOpts(limit=max(0, a.avg_max - 1), count=max(0, a.avg - 1)))
    used = [bank.set_carrier(i, f0=f0) for i, (f0, _) in enumerate(want)]
    host_traces(source, pkg, a, [(idx,) for _, idx in want], lambda i, xs: bank.process(i, xs[0]))
    for i, (_, idx) in enumerate(want):
        two_sided_sk_report(pkg, bank, i, f"zoom sk {names[idx]} @ {used[i]:.12g}", f"zoomsk_{names[idx]}_{used[i]:.9g}", a, merge)
    bank.close()


def iq_sk_streams(pkg, source, a, merge, names):
    """--iq-sk: two traces of every read (host_traces), or two raw f32 files (names None), into one IQ spectral kurtosis cascade per
    stream"""
    want = []
    for z in a.iq_sk:
        parts = z.split(":")
        if len(parts) not in (2, 3) or not parts[0] or not parts[1]:
            raise SystemExit("--iq-sk takes I:Q[:F0]")
        want.append((parts[0], parts[1], float(parts[2]) if len(parts) == 3 else 0.0))
    bank = pkg.IqSkCascadeBank(1 << 9, len(want))
    used, labels = iq_feed(pkg, source, a, bank, want, names, "--iq-sk")
    for c, (li, lq) in enumerate(labels):
        two_sided_sk_report(pkg, bank, c, f"iq sk {li}:{lq} @ {used[c]:.12g}", f"iqsk_{li}__{lq}_{used[c]:.9g}", a, merge)
    bank.close()


def ampm_report(pkg, bank, c, label, stem, a, merge):
    """the read-out of one channel of a ZoomAmPmCascadeBank / IqAmPmCascadeBank: the summary line with the carrier, and
    offset,S_am,S_pm,Re S_ampm,Im S_ampm in the order of the Breaks"""
    if bank.num_stages(c) == 0 or bank.stage_rows(c, 0)[0]["count"] == 0:
        print(f"{label}: no samples")
        return
    power, u, lock = bank.carrier(c)
    s_am, s_pm, s_x, breaks = bank.am_pm(c, opts=merge)
    off = pkg.Break.frequencies(breaks) * a.fs
    print(f"{label}: stages {bank.num_stages(c)} bins {s_am.size} breaks {len(breaks)} carrier power {power:.9g} "
          f"angle {0.5 * np.angle(u):.9g} lock {lock:.9g}")
    lines = [f"{o:.9g},{am:.9g},{pm:.9g},{x.real:.9g},{x.imag:.9g}\n" for o, am, pm, x in zip(off, s_am, s_pm, s_x)]
    if a.csv:
        safe = "".join(ch if ch.isalnum() else "_" for ch in stem)
        with open(os.path.join(a.csv, safe + ".csv"), "w") as f:
            f.writelines(lines)
    else:
        sys.stdout.writelines(lines)


def zoom_ampm_traces(pkg, source, a, merge, names):
    """--zoom-ampm: the named trace of every read (host_traces) into one AM/PM cascade per carrier; no detrend (carrier() reads bin 0)"""
    want = []
    for z in a.zoom_ampm:
        f0, _, tr = z.partition(":")
        want.append((float(f0), trace_arg(tr, names, "--zoom-ampm")))
    bank = pkg.ZoomAmPmCascadeBank(1 << 9, len(want))
    bank.set_avg(pkg.AvgOpts(limit=max(0, a.avg_max - 1), count=max(0, a.avg - 1)))
    used = [bank.set_carrier(i, f0=f0) for i, (f0, _) in enumerate(want)]
    host_traces(source, pkg, a, [(idx,) for _, idx in want], lambda i, xs: bank.process(i, xs[0]))
    for i, (_, idx) in enumerate(want):
        ampm_report(pkg, bank, i, f"zoom am/pm {names[idx]} @ {used[i]:.12g}", f"zoomampm_{names[idx]}_{used[i]:.9g}", a, merge)
    bank.close()


def iq_ampm_streams(pkg, source, a, merge, names):
    """--iq-ampm: two traces of every read (host_traces), or two raw f32 files (names None), into one IQ AM/PM cascade per stream"""
    want = []
    for z in a.iq_ampm:
        parts = z.split(":")
        if len(parts) not in (2, 3) or not parts[0] or not parts[1]:
            raise SystemExit("--iq-ampm takes I:Q[:F0]")
        want.append((parts[0], parts[1], float(parts[2]) if len(parts) == 3 else 0.0))
    bank = pkg.IqAmPmCascadeBank(1 << 9, len(want))
    used, labels = iq_feed(pkg, source, a, bank, want, names, "--iq-ampm", detrend=pkg.Detrend.NONE)
    for c, (li, lq) in enumerate(labels):
        ampm_report(pkg, bank, c, f"iq am/pm {li}:{lq} @ {used[c]:.12g}", f"iqampm_{li}__{lq}_{used[c]:.9g}", a, merge)
    bank.close()


def zoom_pairs(pkg, source, a, merge, names):
    """--zoom-pair: the two named traces of every read (host_traces) into one zoom cross cascade per pair, one carrier on both sides"""
    want = []
    for z in a.zoom_pair:
        parts = z.split(":")
        if len(parts) != 3:
            raise SystemExit("--zoom-pair takes F0:X:Y")
        want.append((float(parts[0]), trace_arg(parts[1], names, "--zoom-pair"), trace_arg(parts[2], names, "--zoom-pair")))
    bank = pkg.ZoomCsdCascadeBank(1 << 9, len(want))
    bank.set_detrend(pkg.Detrend[a.detrend.upper()])
    bank.set_avg(pkg.AvgOpts(limit=max(0, a.avg_max - 1), count=max(0, a.avg - 1)))
    used = [bank.set_carrier(i, f0=f0) for i, (f0, _, _) in enumerate(want)]
    host_traces(source, pkg, a, [(x, y) for _, x, y in want], lambda i, xs: bank.process(i, xs[0], xs[1]))
    for i, (_, x, y) in enumerate(want):
        label = f"zoom pair {names[x]}:{names[y]} @ {used[i]:.12g}"
        if bank.num_stages(i) == 0:
            print(f"{label}: no samples")
            continue
        aup, alo, bup, blo, xup, xlo, breaks = bank.csd(i, merge)
        off = pkg.Break.frequencies(breaks) * a.fs
        coh = pkg.coherence(aup, bup, xup)
        print(f"{label}: stages {bank.num_stages(i)} bins {aup.size} breaks {len(breaks)} median coherence (upper) {np.nanmedian(coh):.6g}")
        lines = [f"{o:.9g},{p:.9g},{q:.9g},{u.real:.9g},{u.imag:.9g},{r:.9g},{t:.9g},{w.real:.9g},{w.imag:.9g}\n"
                 for o, p, q, u, r, t, w in zip(off, aup, bup, xup, alo, blo, xlo)]
        if a.csv:
            safe = "".join(ch if ch.isalnum() else "_" for ch in f"zoompair_{names[x]}__{names[y]}_{used[i]:.9g}")
            with open(os.path.join(a.csv, safe + ".csv"), "w") as f:
                f.writelines(lines)
        else:
            sys.stdout.writelines(lines)
    bank.close()


def iq_feed(pkg, source, a, bank, want, names, opt, detrend=None):
    """settle an IQ bank (AcqOpts, carriers) and feed it `want` = [(I, Q, F0)]: two traces of every read (host_traces), or two raw f32
    files (names None).  detrend: in place of --detrend.  Returns the carriers in use and the (I, Q) labels."""
    bank.set_detrend(pkg.Detrend[a.detrend.upper()] if detrend is None else detrend)
    bank.set_avg(pkg.AvgOpts(limit=max(0, a.avg_max - 1), count=max(0, a.avg - 1)))
    used = [bank.set_carrier(i, f0=f0) for i, (_, _, f0) in enumerate(want)]
    if names is None:
        labels = [(os.path.basename(i), os.path.basename(q)) for i, q, _ in want]
        for c, (pi, pq, _) in enumerate(want):
            if os.path.getsize(pi) != os.path.getsize(pq):
                raise SystemExit(f"{opt}: {pi} and {pq} differ in length")
            with open(pi, "rb") as fi, open(pq, "rb") as fq:
                fed = 0
                while a.max_bytes is None or fed < a.max_bytes:
                    xi, xq = np.fromfile(fi, "<f4", 1 << 20), np.fromfile(fq, "<f4", 1 << 20)
                    if xi.size == 0:
                        break
                    bank.process(c, (xi, xq))
                    fed += xi.nbytes
    else:
        idx = [(trace_arg(i, names, opt), trace_arg(q, names, opt)) for i, q, _ in want]
        labels = [(names[i], names[q]) for i, q in idx]
        host_traces(source, pkg, a, idx, lambda c, xs: bank.process(c, (xs[0], xs[1])))
    return used, labels


def iq_streams(pkg, source, a, merge, names):
    """--iq: two traces of every read (host_traces), or two raw f32 files (names None), into one IQ cascade per stream"""
    want = []
    for z in a.iq:
        parts = z.split(":")
        if len(parts) not in (2, 3) or not parts[0] or not parts[1]:
            raise SystemExit("--iq takes I:Q[:F0]")
        want.append((parts[0], parts[1], float(parts[2]) if len(parts) == 3 else 0.0))
    bank = pkg.IqCascadeBank(1 << 9, len(want))
    used, labels = iq_feed(pkg, source, a, bank, want, names, "--iq")
    for c, (li, lq) in enumerate(labels):
        label = f"iq {li}:{lq} @ {used[c]:.12g}"
        if bank.num_stages(c) == 0:
            print(f"{label}: no samples")
            continue
        up, lo, breaks = bank.psd(c, merge)
        off = pkg.Break.frequencies(breaks) * a.fs
        print(f"{label}: stages {bank.num_stages(c)} bins {up.size} breaks {len(breaks)}")
        lines = [f"{o:.9g},{u:.9g},{w:.9g}\n" for o, u, w in zip(off, up, lo)]
        if a.csv:
            safe = "".join(ch if ch.isalnum() else "_" for ch in f"iq_{li}__{lq}_{used[c]:.9g}")
            with open(os.path.join(a.csv, safe + ".csv"), "w") as f:
                f.writelines(lines)
        else:
            sys.stdout.writelines(lines)
    bank.close()


def iq_pair_feed(pkg, source, a, make_bank, args, names, opt, detrend=None):
    """parse the IA:QA:IB:QB[:F0] arguments of `opt`, settle a bank of make_bank(n, n_pairs) (AcqOpts, one carrier on both sides of a
    pair) and feed it: four traces of every read (host_traces), or four raw f32 files (names None).  detrend: in place of
    --detrend.  Returns the bank, the carriers in use and the four labels of every pair."""
    want = []
    for z in args:
        parts = z.split(":")
        if len(parts) not in (4, 5) or not all(parts[:4]):
            raise SystemExit(opt + " takes IA:QA:IB:QB[:F0]")
        want.append((tuple(parts[:4]), float(parts[4]) if len(parts) == 5 else 0.0))
    bank = make_bank(1 << 9, len(want))
    bank.set_detrend(pkg.Detrend[a.detrend.upper()] if detrend is None else detrend)
    bank.set_avg(pkg.AvgOpts(limit=max(0, a.avg_max - 1), count=max(0, a.avg - 1)))
    used = [bank.set_carrier(i, f0=f0) for i, (_, f0) in enumerate(want)]
    if names is None:
        labels = [tuple(os.path.basename(f) for f in files) for files, _ in want]
        for p, (files, _) in enumerate(want):
            if len({os.path.getsize(f) for f in files}) != 1:
                raise SystemExit(opt + ": " + ", ".join(files) + " differ in length")
            fh = [open(f, "rb") for f in files]
            fed = 0
            while a.max_bytes is None or fed < a.max_bytes:
                xs = [np.fromfile(f, "<f4", 1 << 20) for f in fh]
                if xs[0].size == 0:
                    break
                bank.process(p, (xs[0], xs[1]), (xs[2], xs[3]))
                fed += xs[0].nbytes
            for f in fh:
                f.close()
    else:
        idx = [tuple(trace_arg(t, names, opt) for t in tr) for tr, _ in want]
        labels = [tuple(names[i] for i in four) for four in idx]
        host_traces(source, pkg, a, idx, lambda p, xs: bank.process(p, (xs[0], xs[1]), (xs[2], xs[3])))
    return bank, used, labels


def iq_pairs(pkg, source, a, merge, names):
    """--iq-pair: four traces of every read, or four raw f32 files (names None), into one IQ cross cascade per pair (iq_pair_feed)"""
    bank, used, labels = iq_pair_feed(pkg, source, a, pkg.IqCsdCascadeBank, a.iq_pair, names, "--iq-pair")
    for p, lab in enumerate(labels):
        label = f"iq pair {lab[0]}:{lab[1]}:{lab[2]}:{lab[3]} @ {used[p]:.12g}"
        if bank.num_stages(p) == 0:
            print(f"{label}: no samples")
            continue
        aup, alo, bup, blo, xup, xlo, breaks = bank.csd(p, merge)
        off = pkg.Break.frequencies(breaks) * a.fs
        coh = pkg.coherence(aup, bup, xup)
        print(f"{label}: stages {bank.num_stages(p)} bins {aup.size} breaks {len(breaks)} median coherence (upper) {np.nanmedian(coh):.6g}")
        lines = [f"{o:.9g},{u:.9g},{v:.9g},{x.real:.9g},{x.imag:.9g},{r:.9g},{t:.9g},{w.real:.9g},{w.imag:.9g}\n"
                 for o, u, v, x, r, t, w in zip(off, aup, bup, xup, alo, blo, xlo)]
        if a.csv:
            safe = "".join(ch if ch.isalnum() else "_" for ch in f"iqpair_{lab[0]}__{lab[1]}__{lab[2]}__{lab[3]}_{used[p]:.9g}")
            with open(os.path.join(a.csv, safe + ".csv"), "w") as f:
                f.writelines(lines)
        else:
            sys.stdout.writelines(lines)
    bank.close()


def ampm_pair_report(pkg, bank, p, label, stem, a, merge):
    """the read-out of one pair of a ZoomAmPmCsdCascadeBank / IqAmPmCsdCascadeBank: the summary line with the carriers, and offset,
    then Re and Im of s_am, s_pm, s_am_pm, s_pm_am in the order of the Breaks"""
    if bank.num_stages(p) == 0 or bank.stage_rows(p, 0)[0]["count"] == 0:
        print(f"{label}: no samples")
        return
    p_ab, w, q, lock_w, lock_q = bank.carriers(p)
    *spectra, breaks = bank.am_pm_cross(p, opts=merge)
    off = pkg.Break.frequencies(breaks) * a.fs
    print(f"{label}: stages {bank.num_stages(p)} bins {spectra[0].size} breaks {len(breaks)} p_ab {p_ab:.9g} "
          f"angle w {np.angle(w):.9g} angle q {np.angle(q):.9g} lock_w {lock_w:.9g} lock_q {lock_q:.9g}")
    lines = [f"{o:.9g}," + ",".join(f"{v.real:.9g},{v.imag:.9g}" for v in row) + "\n" for o, *row in zip(off, *spectra)]
    if a.csv:
        safe = "".join(ch if ch.isalnum() else "_" for ch in stem)
        with open(os.path.join(a.csv, safe + ".csv"), "w") as f:
            f.writelines(lines)
    else:
        sys.stdout.writelines(lines)


def zoom_ampm_pairs(pkg, source, a, merge, names):
    """--zoom-ampm-pair: the two named traces of every read (host_traces) into one AM/PM cross cascade per pair, one carrier on both
    sides; no detrend (carriers() reads bin 0)"""
    want = []
    for z in a.zoom_ampm_pair:
        parts = z.split(":")
        if len(parts) != 3:
            raise SystemExit("--zoom-ampm-pair takes F0:X:Y")
        want.append((float(parts[0]), trace_arg(parts[1], names, "--zoom-ampm-pair"), trace_arg(parts[2], names, "--zoom-ampm-pair")))
    bank = pkg.ZoomAmPmCsdCascadeBank(1 << 9, len(want))
    bank.set_avg(pkg.AvgOpts(limit=max(0, a.avg_max - 1), count=max(0, a.avg - 1)))
    used = [bank.set_carrier(i, f0=f0) for i, (f0, _, _) in enumerate(want)]
    host_traces(source, pkg, a, [(x, y) for _, x, y in want], lambda i, xs: bank.process(i, xs[0], xs[1]))
    for i, (_, x, y) in enumerate(want):
        ampm_pair_report(pkg, bank, i, f"zoom am/pm pair {names[x]}:{names[y]} @ {used[i]:.12g}",
                         f"zoomampmpair_{names[x]}__{names[y]}_{used[i]:.9g}", a, merge)
    bank.close()


def iq_ampm_pairs(pkg, source, a, merge, names):
    """--iq-ampm-pair: four traces of every read, or four raw f32 files (names None), into one IQ AM/PM cross cascade per pair"""
    bank, used, labels = iq_pair_feed(pkg, source, a, pkg.IqAmPmCsdCascadeBank, a.iq_ampm_pair, names, "--iq-ampm-pair",
                                      detrend=pkg.Detrend.NONE)
    for p, lab in enumerate(labels):
        ampm_pair_report(pkg, bank, p, f"iq am/pm pair {lab[0]}:{lab[1]}:{lab[2]}:{lab[3]} @ {used[p]:.12g}",
                         f"iqampmpair_{lab[0]}__{lab[1]}__{lab[2]}__{lab[3]}_{used[p]:.9g}", a, merge)
    bank.close()


def int_feeds(pkg, a):
    """--sample-format s16 / s8: raw integer files through process_int, 2^20 units a call; one object per option given"""
    dtype = np.dtype("<i2" if a.sample_format == "s16" else "i1")
    merge = pkg.MergeOpts(keep_overlap=a.keep_overlap, min_count=a.avg_min, keep_transition_band=a.keep_transition_band)
    if a.csv:
        os.makedirs(a.csv, exist_ok=True)

    def settle(bank):
        bank.set_detrend(pkg.Detrend[a.detrend.upper()])
        bank.set_avg(pkg.AvgOpts(limit=max(0, a.avg_max - 1), count=max(0, a.avg - 1)))
        return bank

    def feed(files, per_unit, opt, process):
        """the files in step, 2^20 units a read; per_unit integers a unit (2: interleaved pairs)"""
        if len({os.path.getsize(f) for f in files}) != 1:
            raise SystemExit(f"{opt}: " + ", ".join(files) + " differ in length")
        if os.path.getsize(files[0]) % (per_unit * dtype.itemsize):
            raise SystemExit(f"{opt}: {files[0]} does not hold whole units of {per_unit * dtype.itemsize} bytes")
        fh = [open(f, "rb") for f in files]
        fed = 0
        while a.max_bytes is None or fed < a.max_bytes:
            xs = [np.fromfile(f, dtype, per_unit << 20) for f in fh]
            if xs[0].size == 0:
                break
            process([x.reshape(-1, 2) if per_unit == 2 else x for x in xs])
            fed += xs[0].nbytes
        for f in fh:
            f.close()

    def emit(name, lines):
        if a.csv:
            safe = "".join(ch if ch.isalnum() else "_" for ch in name)
            with open(os.path.join(a.csv, safe + ".csv"), "w") as f:
                f.writelines(lines)
        else:
            sys.stdout.writelines(lines)

    def single(bank, label, stem):
        if bank.num_stages(0) == 0:
            print(f"{label}: no samples")
            return
        up, lo, breaks = bank.psd(0, merge)
        off = pkg.Break.frequencies(breaks) * a.fs
        print(f"{label}: stages {bank.num_stages(0)} bins {up.size} breaks {len(breaks)}")
        emit(stem, [f"{o:.9g},{u:.9g},{w:.9g}\n" for o, u, w in zip(off, up, lo)])

    def pair(bank, label, stem):
        if bank.num_stages(0) == 0:
            print(f"{label}: no samples")
            return
        aup, alo, bup, blo, xup, xlo, breaks = bank.csd(0, merge)
        off = pkg.Break.frequencies(breaks) * a.fs
        coh = pkg.coherence(aup, bup, xup)
        print(f"{label}: stages {bank.num_stages(0)} bins {aup.size} breaks {len(breaks)} median coherence (upper) {np.nanmedian(coh):.6g}")
        emit(stem, [f"{o:.9g},{p:.9g},{q:.9g},{u.real:.9g},{u.imag:.9g},{r:.9g},{t:.9g},{w.real:.9g},{w.imag:.9g}\n"
                    for o, p, q, u, r, t, w in zip(off, aup, bup, xup, alo, blo, xlo)])

    if a.raw:  # the plain spectrum: the lines of the f32 --raw
        bank = settle(pkg.PsdCascadeBank(1 << 9, 1))
        feed([a.raw], 1, "--raw", lambda xs: bank.process_int(0, xs[0], a.scale))
        if bank.num_stages(0) == 0:
            print("raw: no samples")
        else:
            psd, breaks = bank.psd(0, merge)
            rms, xy = pkg.trace_plot(psd, pkg.Break.frequencies(breaks), fs=a.fs, integrate=a.integrate,
                                     integral_start=a.integral_start * a.fs, integral_end=a.integral_end * a.fs)
            top = bank.stage_info(0, 0)["count"]
            print(f"raw: stages {bank.num_stages(0)} top-stage averages {top} bins {psd.size} breaks {len(breaks)} rms {rms:.9g}")
            if a.csv:
                emit("raw", [f"{x:.9g},{y:.9g}\n" for x, y in xy])
        bank.close()
    for z in a.pair:  # the lines of the f32 --pair
        parts = z.split(":")
        if len(parts) != 2 or not all(parts):
            raise SystemExit("--pair takes FILEX:FILEY with --sample-format s16 / s8")
        bank = settle(pkg.CsdCascadeBank(1 << 9, 1))
        feed(parts, 1, "--pair", lambda xs: bank.process_int(0, xs[0], xs[1], a.scale))
        x, y = (os.path.basename(f) for f in parts)
        if bank.num_stages(0) == 0:
            print(f"{x}:{y}: no samples")
        else:
            sxx, syy, sxy, breaks = bank.csd(0, merge)
            freqs = pkg.Break.frequencies(breaks) * a.fs
            coh, h1 = pkg.coherence(sxx, syy, sxy), pkg.transfer(sxx, sxy)
            print(f"{x}:{y}: bins {sxx.size} median coherence {np.nanmedian(coh):.6g}")
            if a.csv:
                emit(f"pair_{x}__{y}", [f"{fr:.9g},{abs(h):.9g},{np.angle(h):.9g},{c:.9g}\n" for fr, h, c in zip(freqs, h1, coh)])
        bank.close()
    for z in a.zoom:
        f0, _, path = z.partition(":")
        if not path:
            raise SystemExit("--zoom takes F0:FILE with --sample-format s16 / s8")
        bank = settle(pkg.ZoomCascadeBank(1 << 9, 1))
        used = bank.set_carrier(0, f0=float(f0))
        feed([path], 1, "--zoom", lambda xs: bank.process_int(0, xs[0], a.scale))
        base = os.path.basename(path)
        single(bank, f"zoom {base} @ {used:.12g}", f"zoom_{base}_{used:.9g}")
        bank.close()
    for z in a.zoom_pair:
        parts = z.split(":")
        if len(parts) != 3 or not all(parts):
            raise SystemExit("--zoom-pair takes F0:FILEA:FILEB with --sample-format s16 / s8")
        bank = settle(pkg.ZoomCsdCascadeBank(1 << 9, 1))
        used = bank.set_carrier(0, f0=float(parts[0]))
        feed(parts[1:], 1, "--zoom-pair", lambda xs: bank.process_int(0, xs[0], xs[1], a.scale))
        x, y = (os.path.basename(f) for f in parts[1:])
        pair(bank, f"zoom pair {x}:{y} @ {used:.12g}", f"zoompair_{x}__{y}_{used:.9g}")
        bank.close()
    for z in a.iq:
        path, _, f0 = z.partition(":")
        bank = settle(pkg.IqCascadeBank(1 << 9, 1))
        used = bank.set_carrier(0, f0=float(f0) if f0 else 0.0)
        feed([path], 2, "--iq", lambda xs: bank.process_int(0, xs[0], a.scale))
        base = os.path.basename(path)
        single(bank, f"iq {base} @ {used:.12g}", f"iq_{base}_{used:.9g}")
        bank.close()
    for z in a.iq_pair:
        parts = z.split(":")
        if len(parts) not in (2, 3) or not all(parts[:2]):
            raise SystemExit("--iq-pair takes FILEA:FILEB[:F0] with --sample-format s16 / s8")
        bank = settle(pkg.IqCsdCascadeBank(1 << 9, 1))
        used = bank.set_carrier(0, f0=float(parts[2]) if len(parts) == 3 else 0.0)
        feed(parts[:2], 2, "--iq-pair", lambda xs: bank.process_int(0, xs[0], xs[1], a.scale))
        x, y = (os.path.basename(f) for f in parts[:2])
        pair(bank, f"iq pair {x}:{y} @ {used:.12g}", f"iqpair_{x}__{y}_{used:.9g}")
        bank.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
