// cpp_mirror_check.cpp -- the reference's stream_test flow (src/bin/stream_test.rs:38-66) written
// against the C++ mirror stabilizer-stream_amd/cpp/psd_cascade.hpp: four PsdCascade<512>, traces fed
// in small chunks, clone, psd(&MergeOpts::default()), Break::frequencies.  The numbers are those of
// the reference's own test (src/psd.rs:602-643): 2^16 samples of unit-variance white noise, default
// detrend, every included bin within 10/sqrt(count) of PSD = 2 (trace 0 runs Detrend::Midpoint as
// stream_test does, which is exercised but not held to that bound: on white noise it adds a random
// DC level by construction).
// Needs a GPU to run; building it is the check that the mirror matches the C ABI.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../../stabilizer-stream_amd/cpp/psd_cascade.hpp"
#include "../../stabilizer-stream_amd/cpp/source.hpp"

using namespace stabilizer_stream;

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : "/tmp"; // (the test passes a private directory)
    constexpr size_t N = 1 << 9;
    std::vector<PsdCascade<N>> dec;
    for (int i = 0; i < 4; ++i)
        dec.emplace_back();
    dec[0].set_detrend(Detrend::Midpoint); // src/bin/stream_test.rs:41
    std::mt19937 rng(0x7654321);
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    std::vector<float> x(176); // one dual-iir frame's worth per trace (22 batches x 8)
    const size_t total = size_t(1) << 16; // src/psd.rs:603
    for (size_t done = 0; done < total; done += x.size())
        for (auto &d : dec) {
            for (auto &v : x)
                v = (u(rng) - 0.5f) * std::sqrt(12.0f); // src/psd.rs:604-606
            d.process(x);
        }
    PsdCascade<N> copy = dec[1]; // Clone (src/psd.rs:399)
    const auto [y, b] = copy.psd(MergeOpts{});
    const auto f = Break::frequencies(b);
    if (b.empty() || y.size() != f.size() || f.front() != 0.0f || f.back() != 0.5f) {
        std::fprintf(stderr, "bad shape: %zu breaks, %zu bins, %zu freqs\n", b.size(), y.size(), f.size());
        return 1;
    }
    int bad = 0;
    for (const auto &br : b) {
        if (!br.include)
            continue;
        const double tol = 10.0 / std::sqrt((double)br.count); // the reference's own bound (src/psd.rs:639-642)
        for (size_t k = br.start; k < br.start + (br.bins.second - br.bins.first); ++k)
            if (std::fabs(y[k] * 0.5 - 1.0) > tol)
                ++bad;
        std::printf("stage fft %zu x%zu: count %u, bins %zu..%zu, rbw %.3g\n", br.fft_size, br.decimation, br.count,
                    br.bins.first, br.bins.second, br.rbw());
    }
    // the tail of stream_test (src/bin/stream_test.rs:61-71): FDEV sweep over tau = 1, 2, 4, ... on the merged PSD
    {
        const Var var{.x_exp = -2, .sinx_exp = 4, .clip = 1.0f, .dc_cut = 1}; // VarBuilder::default().dc_cut(1).clip(1.0)
        int n_tau = 0;
        for (float tau = 1.0f; tau <= (float)(b.front().effective_fft_size() / 2); tau *= 2.0f) {
            const float v = var.eval(y, f, tau);
            if (!(v >= 0.0f) || !std::isfinite(std::sqrt(v)))
                ++bad;
            // white frequency-noise level: S_phi = 2 flat => the main-lobe variance falls with tau; just sanity here,
            // the bit-exact comparison with the restatement is tests/test_oracle_reference.py
            if (n_tau < 3)
                std::printf("fdev(tau=%g) = %.6g\n", tau, std::sqrt(v));
            ++n_tau;
        }
        std::printf("fdev sweep: %d taus\n", n_tau);
        const auto [rms, pts] = trace_plot(y, f, 1.0f, true, 0.0f, 1.0f); // Trace::plot, whole band
        if (std::fabs(rms - 1.0f) > 0.05f || pts.size() + 1 != f.size())
            ++bad;
        std::printf("integrated rms %.4f over %zu plot points\n", rms, pts.size());
    }
    // the reference's own single-stage test (src/psd.rs:615-632) through the Psd<N> mirror
    {
        std::vector<float> xs(total), ys(total >> 3);
        for (auto &v : xs)
            v = (u(rng) - 0.5f) * std::sqrt(12.0f);
        Psd<N> s(N, Window<N>::hann()); // Psd::<N>::new(FftPlanner::new().plan_fft_forward(N), Arc::new(Window::hann()))
        const auto out = s.process(xs, ys);
        if (out.size() != (xs.size() >> 3) - (size_t)psdc_hbf_response_length(3)) { // :622
            std::fprintf(stderr, "Psd::process returned %zu items\n", out.size());
            ++bad;
        }
        const float g = 1.0f / s.gain();
        for (const float p : s.spectrum())
            if (std::fabs(p * g * 0.5 - 1.0) > 10.0 / std::sqrt((double)s.count())) // :623-632
                ++bad;
        std::printf("Psd<%zu>: %zu outputs, count %u, %zu pending\n", N, out.size(), s.count(), s.buf().size());
        // a Window<N> built by the caller (pub fields, src/psd.rs:12-20): Hann's weights rebuilt by hand must be
        // recognised as Hann (same fused kernels, same bits); a flat-top-ish table must go through and normalise
        Window<N> mine;
        mine.win.resize(N);
        const float df = 3.14159265358979323846f / (float)N;
        for (size_t i = 0; i < N; ++i) {
            const float sn = std::sin(df * (float)i);
            mine.win[i] = sn * sn;
        }
        mine.power = 0.25f;
        mine.nenbw = 1.5f;
        mine.overlap = N / 2;
        Psd<N> s2(N, mine);
        std::vector<float> y2(total >> 3);
        s2.process(xs, y2);
        if (s2.spectrum() != s.spectrum() || s2.count() != s.count())
            ++bad;
        bool threw = false;
        try {
            Psd<N> wrong(N / 2, mine); // assert_eq!(N, fft.len()) src/psd.rs:139
        } catch (const std::invalid_argument &) {
            threw = true;
        }
        if (!threw)
            ++bad;
        double m1 = 0.0, m2 = 0.0;
        for (size_t i = 0; i < N; ++i) { // Hamming, hop N/4
            mine.win[i] = 0.54f - 0.46f * std::cos(2.0f * df * (float)i);
            m1 += mine.win[i];
            m2 += (double)mine.win[i] * mine.win[i];
        }
        m1 /= N;
        m2 /= N;
        mine.power = (float)(m1 * m1);
        mine.nenbw = (float)(m2 / (m1 * m1));
        mine.overlap = 3 * N / 4;
        PsdCascade<N> hc(mine);
        hc.process(xs);
        const auto [ph, bh] = hc.psd(MergeOpts{});
        size_t off = 0;
        for (const Break &b : bh) {
            const size_t len = b.include ? b.bins.second - b.bins.first : 0;
            for (size_t i = 0; i < len; ++i)
                if (std::fabs(ph[off + i] * 0.5 - 1.0) > 10.0 / std::sqrt((double)b.count)) // white noise reads PSD = 2 whatever the window
                    ++bad;
            off += len;
        }
        // the packed read-out stitches to the same bits
        const auto rec = hc.pack_readout();
        const auto [pr, brr] = psd_from_readout(rec);
        if (pr != ph || brr.size() != bh.size())
            ++bad;
        // ... and so does the record padded to the channel count of a larger shard (psdc_pack_pad)
        const auto rec3 = pad_readout(rec, N, 3);
        const auto [pp, brp] = psd_from_readout(rec3);
        if (pp != ph || brp.size() != bh.size() || !psd_from_readout(rec3, 2).first.empty())
            ++bad;
        std::printf("caller-built windows: Hann table recognised, Hamming cascade %zu stages, record %zu bytes\n", bh.size(), rec.size());
    }
    // the batched feeder (cpp/source.hpp): a raw f32 file as stream_to_raw writes it (src/bin/stream_to_raw.rs:24-25),
    // ingested in 100 kB reads through Source::feed, must give the same PSD as process() on the same samples
    {
        std::vector<float> xs(total);
        for (auto &v : xs)
            v = (u(rng) - 0.5f) * std::sqrt(12.0f);
        const std::string path = dir + "/psd_cpp_mirror_raw.f32";
        std::FILE *fp = std::fopen(path.c_str(), "wb");
        if (!fp) {
            std::printf("cannot write %s\n", path.c_str());
            return 1;
        }
        std::fwrite(xs.data(), 4, xs.size(), fp);
        std::fclose(fp);
        SourceOpts so;
        so.raw = path;
        Source src(so);
        PsdCascade<N> a, bref;
        size_t fed = 0;
        while (size_t nb = src.feed(a.handle(), 100000))
            fed += nb;
        bref.process(xs);
        const auto [pa, ba] = a.psd(MergeOpts{});
        const auto [pb, bb] = bref.psd(MergeOpts{});
        if (fed != 4 * xs.size() || pa.size() != pb.size() || ba.size() != bb.size())
            ++bad;
        for (size_t k = 0; k < pa.size() && k < pb.size(); ++k)
            if (std::fabs(pa[k] - pb[k]) > 4e-6f * pb[k])
                ++bad;
        std::remove(path.c_str());
        std::printf("Source::feed: %zu bytes, %zu bins equal to process()\n", fed, pa.size());
    }
    bool threw = false;
    try {
        copy.set_detrend(Detrend::Linear); // unimplemented!() in the reference (src/psd.rs:110)
    } catch (const std::runtime_error &) {
        threw = true;
    }
    std::printf("%zu stages, %zu bins, %d out of bound, Linear %s\n", b.size(), y.size(), bad, threw ? "throws" : "ACCEPTED");
    return (bad == 0 && threw) ? 0 : 1;
}
