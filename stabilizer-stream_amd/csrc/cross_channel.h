// cross_channel.h -- one channel of the cross-spectral kernels, shared by cross.hip (pairs), csm.hip (groups of m channels) and
// zoom.hip / zoom_cross.hip (the I / Q pair of a mixed-down channel):
// load, detrend and window two consecutive segments of a channel, transform them as one complex signal and leave the spectrum
// in natural order in an LDS frame (cross_fft.h) -- or, for the zoom kernels, leave nothing in the frame and add |Z|^2 of the
// thread's bins to its registers, or hand the bins themselves back.  The workgroup shape (CrossCfg) is plain constants; the rest
// is device code.
#pragma once
#include "cross_fft.h"

namespace psdk {

// The workgroup of a segment kernel as closed formulas of n (a power of two, 64 ... 4096): a team of n / 16 threads transforms a
// segment, a workgroup is as many teams as fill 128 threads (one team from n = 2048 up), and a tile gives every team one
// segment pair.  The host side reads them too (cross_block_threads, *_segments_per_tile).
constexpr bool seg_supported(int n) { return n >= 64 && n <= 4096 && (n & (n - 1)) == 0; }
constexpr int seg_team(int n) { return n / 16; }
constexpr int seg_block(int n) { return seg_team(n) > 128 ? seg_team(n) : 128; }
constexpr int seg_teams(int n) { return seg_block(n) / seg_team(n); }
constexpr int seg_spt(int n) { return 2 * seg_teams(n); } // fine tiles keep the workgroups of a launch even

template <int N>
struct CrossCfg {
    using Plan = FftPlan<N>;
    static constexpr int E = Plan::E;
    static constexpr int TEAM = seg_team(N);
    static constexpr int BLOCK = seg_block(N);
    static constexpr int TEAMS = seg_teams(N);
    static constexpr int SPT = seg_spt(N); // segments per tile: one pair a team
    static constexpr int WAVES = BLOCK / 64;
    static constexpr int H = N / 2 + 1;
    static constexpr int FRAME = LdsFrame<N>::SIZE;
    static_assert(E == 16 && TEAM == Plan::TEAM, "cross kernel: sixteen elements a thread");
    static_assert(H <= FRAME, "partial rows reuse the frames' LDS");
};
static_assert(CrossCfg<64>::TEAMS == 32 && CrossCfg<128>::TEAMS == 16 && CrossCfg<256>::TEAMS == 8 && CrossCfg<512>::TEAMS == 4 &&
                  CrossCfg<1024>::TEAMS == 2 && CrossCfg<2048>::TEAMS == 1 && CrossCfg<4096>::TEAMS == 1 && CrossCfg<4096>::BLOCK == 256,
              "the seven sizes: 128 threads a workgroup, one team of 256 at n = 4096");

#ifdef __HIPCC__
template <class Job>
__device__ __forceinline__ float cross_amp(const Job &job, int step)
{
    const int m = step > job.is_m1 ? step : job.is_m1;
    const int na = job.nb - m;
    if (na <= 0)
        return 1.0f;
    return (float)exp2(0.5 * (double)na * job.log2_gamma);
}

template <int TEAM>
__device__ __forceinline__ void xteam_sync()
{
    if constexpr (TEAM <= 64) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

template <int N, int P>
__device__ __forceinline__ void xfft_run(int t, cf *v, cf *frame, const cf *__restrict__ tw)
{
    using PI = PassInfo<N, P>;
    if constexpr (P == 0)
        xteam_sync<PI::TEAM>(); // the frame's previous readers (separation) are done
    xfft_pass<N, P>(t, v, frame, tw);
    xteam_sync<PI::TEAM>();
    if constexpr (!PI::LAST)
        xfft_run<N, P + 1>(t, v, frame, tw);
}

// Load, detrend, window one channel's segment pair (a = segment la, b = la + 1) into v, transform, and leave the spectrum of
// z = a + i b in natural order in `frame`.
// ZOOM = true (zoom.hip): segment b is read from the stream srcq in place of src -- a and b are the I and Q of ONE segment --
// and the spectrum is not stored: |Z|^2 of the thread's bins is added to pw, pw[s] being bin freq_of_slot<N>(t, s).
// KEEP = true (zoom_cross.hip, with ZOOM): nothing is summed; the thread's bins are handed back in zout, in the order of pw.
template <int N, bool ZOOM = false, bool KEEP = false>
__device__ __forceinline__ void cross_channel(const float *__restrict__ src, long long ofs_la, long long ofs_lb, bool act_a,
                                              bool act_b, int detrend, float ampa, float ampb, int t, int team, cf *frame,
                                              float *red, const float *__restrict__ win, const cf *__restrict__ tw,
                                              const float *srcq = nullptr, float *pw = nullptr, cf *zout = nullptr)
{
    static_assert(ZOOM || !KEEP, "the bins are handed back by the zoom kernels only");
    const float *srcb = ZOOM ? srcq : src;
    using Cfg = CrossCfg<N>;
    using P0 = PassInfo<N, 0>;
    constexpr int E = Cfg::E, TEAM = Cfg::TEAM;
    float ra[E], rb[E];
#pragma unroll
    for (int i = 0; i < P0::NB; ++i)
#pragma unroll
        for (int m = 0; m < P0::R; ++m) {
            const int nidx = P0::elem(t, i, m);
            const float va = src[ofs_la + nidx], vb = srcb[ofs_lb + nidx];
            ra[i * P0::R + m] = act_a ? va : 0.0f;
            rb[i * P0::R + m] = act_b ? vb : 0.0f;
        }
    // detrend as welch_kernel: (x - o) - (m + n s)
    float oa = 0.0f, ob = 0.0f, ma = 0.0f, mb = 0.0f;
    slope2 sa = {0.0f, 0.0f}, sb = {0.0f, 0.0f};
    if (detrend == 1) { // Midpoint src/psd.rs:87-93
        const float va = src[ofs_la + N / 2], vb = srcb[ofs_lb + N / 2];
        oa = act_a ? va : 0.0f;
        ob = act_b ? vb : 0.0f;
    } else if (detrend == 2) { // Span :94-102
        const float a0 = src[ofs_la], a1 = src[ofs_la + N - 1], b0 = srcb[ofs_lb], b1 = srcb[ofs_lb + N - 1];
        if (act_a) {
            oa = a0;
            sa = span_slope(oa, a1, N);
        }
        if (act_b) {
            ob = b0;
            sb = span_slope(ob, b1, N);
        }
    } else if (detrend == 3) { // Mean :103-109: o = f32 mean, m = mean of x - o
        auto team_sum2 = [&](float &pa, float &pb) __attribute__((always_inline)) {
            constexpr int W = TEAM < 64 ? TEAM : 64;
#pragma unroll
            for (int o = W / 2; o > 0; o >>= 1) {
                pa += __shfl_xor(pa, o);
                pb += __shfl_xor(pb, o);
            }
            if constexpr (TEAM > 64) { // one team a workgroup: combine its wavefronts through LDS
                constexpr int WPT = TEAM / 64;
                const int w = threadIdx.x >> 6;
                if ((threadIdx.x & 63) == 0) {
                    red[2 * w] = pa;
                    red[2 * w + 1] = pb;
                }
                __syncthreads();
                pa = 0.0f;
                pb = 0.0f;
                for (int i = 0; i < WPT; ++i) {
                    pa += red[2 * (team * WPT + i)];
                    pb += red[2 * (team * WPT + i) + 1];
                }
                __syncthreads();
            }
        };
        float pa = 0.0f, pb = 0.0f;
#pragma unroll
        for (int s = 0; s < E; ++s) {
            pa += ra[s];
            pb += rb[s];
        }
        team_sum2(pa, pb);
        oa = pa / (float)N;
        ob = pb / (float)N;
        pa = 0.0f;
        pb = 0.0f;
#pragma unroll
        for (int s = 0; s < E; ++s) {
            pa += ra[s] - oa;
            pb += rb[s] - ob;
        }
        team_sum2(pa, pb);
        ma = pa / (float)N;
        mb = pb / (float)N;
    }
    cf v[E];
#pragma unroll
    for (int i = 0; i < P0::NB; ++i)
#pragma unroll
        for (int m = 0; m < P0::R; ++m) {
            const int s = i * P0::R + m;
            const int nidx = P0::elem(t, i, m);
            const float w = win[nidx];
            float a = ra[s], b = rb[s];
            if (detrend != 0) {
                a = fmaf(-(float)nidx, sa.lo, fmaf(-(float)nidx, sa.hi, a - oa)) - ma;
                b = fmaf(-(float)nidx, sb.lo, fmaf(-(float)nidx, sb.hi, b - ob)) - mb;
            }
            v[s].re = a * w * ampa;
            v[s].im = b * w * ampb;
        }
    xfft_run<N, 0>(t, v, frame, tw);
    if constexpr (KEEP) {
#pragma unroll
        for (int s = 0; s < E; ++s)
            zout[s] = v[s];
    } else if constexpr (ZOOM) {
#pragma unroll
        for (int s = 0; s < E; ++s)
            pw[s] += v[s].re * v[s].re + v[s].im * v[s].im;
    } else {
        store_natural<N>(t, v, frame);
    }
}
#endif // __HIPCC__

} // namespace psdk
