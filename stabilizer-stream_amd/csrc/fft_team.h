// fft_team.h -- N-point forward complex FFT by a TEAM of N/16 lanes of one
// wavefront (N = 256, 512, 1024 -> 16, 32, 64 lanes; 4, 2, 1 independent FFTs
// per wavefront), 16 elements per lane, radix (4, N/64, 16) decimation in
// frequency, two exchanges through a padded LDS frame private to the team.
//
// Why this plan: the pass-0 butterflies of team-lane tl work on elements
// n = 4 tl + c + (N/4) m (c, m = 0..3), exactly what four 16-byte loads
// x[(N/4) m + 4 tl .. +3] deliver -- the sample stream goes HBM -> VGPR in
// dwordx4 pieces with no staging copy.  After pass 2, register slot q of
// team-lane tl holds bin  k = q0 + 4 q1 + 4 R1 q  with q0 = tl / R1,
// q1 = tl % R1, R1 = N/64.  Only |X|^2 is consumed (src/psd.rs:228-233).
//
// Frame: physical = idx + idx/16 (N + N/16 elements).  Every 8-byte LDS access
// of every pass is bank-conflict free under the gfx950 rules, also across the
// teams of one wavefront (tests/host/fft_emul.cpp counts them), and every
// address is lane_base + constant, so the constants ride in the DS offset field.
//
// N = 1024 (the team is the whole wavefront) runs its SECOND exchange differently
// (PSDK_ADDTID, store1_planes / load2_planes below): slot q of every lane goes to
// row q of a re plane and of an im plane, 64 consecutive dwords a row -- the
// address form of ds_write_addtid_b32, which has no address register and so moves
// one dword over the store path (2 cycles) where the paired 16-byte stores the
// backend makes of store1 move five (~13): 32 x 2 = 64 store-path cycles instead
// of 8 x 13.  The reader's sixteen elements are then consecutive dwords of a row:
// 4 + 4 ds_read_b128 (4 LDS cycles each, as many as the sixteen ds_read_b64 they
// replace).  The FIRST exchange keeps the cf frame: its reader's elements are a
// stride of four apart in any such layout, so planes would double its reads.
#pragma once
#include "fft_core.h"

// 1: add-tid stores in the N = 1024 team kernel (second FFT exchange, stage-A
// outputs); 0: the cf frame and ds_write_b32, the form of every other size (A/B)
#ifndef PSDK_ADDTID
#define PSDK_ADDTID 1
#endif
// 1: the first exchange's stores of the N = 1024 team kernel as sixteen single
// ds_write_b64 (store0<true>); 0: left to the backend, which pairs them (A/B)
#ifndef PSDK_ST0_SINGLE
#define PSDK_ST0_SINGLE 1
#endif

namespace psdk {

template <int N>
struct TeamFft {
    static_assert(N == 256 || N == 512 || N == 1024, "team FFT sizes");
    static constexpr int TEAM = N / 16;       // lanes per FFT
    static constexpr int TPW = 64 / TEAM;     // FFTs per wavefront
    static constexpr int R1 = N / 64;         // pass-1 radix (4, 8, 16)
    static constexpr int NB1 = 16 / R1;       // pass-1 butterflies per lane
    static constexpr int L1 = N / 4;          // pass-1 sub-transform length
    static constexpr int FRAME = N + N / 16;  // padded frame, complex elements
    static constexpr int TW0_SIZE = 4 * TEAM; // W_N^(4 tl + c), [c][tl]
    static constexpr int TW1_SIZE = (R1 - 1) * 16; // W_L1^(s q), [(q-1)][s]

    static PSDK_HD int swz(int idx) { return idx + (idx >> 4); }

    static PSDK_HD int freq_of(int tl, int q) { return tl / R1 + 4 * (tl % R1) + 4 * R1 * q; }

    // pass 0: v[4m + c] holds z[4 tl + c + (N/4) m]; afterwards v[4q + c] is output q of
    // butterfly s = 4 tl + c times W_N^(s q).  Only W^s is tabulated (tw0[c*TEAM + tl]);
    // W^2s and W^3s are formed by multiplication (LDS space goes to the decimator state).
    static PSDK_HD void pass0(int tl, cf *v, const cf *tw0)
    {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            cf b[4] = {v[c], v[4 + c], v[8 + c], v[12 + c]};
            Dft<4>::run(b);
            const cf w1 = tw0[c * TEAM + tl]; // (plain loads: see pass1)
            const cf w2 = cmul(w1, w1);
            const cf w3 = cmul(w2, w1);
            v[c] = b[0];
            v[4 + c] = cmul(b[1], w1);
            v[8 + c] = cmul(b[2], w2);
            v[12 + c] = cmul(b[3], w3);
        }
    }

    // ONE: sixteen single 8-byte stores (lds_st), every constant in the 16-bit offset field; otherwise the backend pairs
    // them into eight ds_write2_b64 and rebuilds the addresses its 8-bit offsets do not reach
    template <bool ONE = false>
    static PSDK_HD void store0(int tl, const cf *v, cf *frame)
    {
        cf *base = frame + (4 * tl + (tl >> 2)); // swz(q L1 + 4 tl + c) = base + q (L1 + L1/16) + c
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if constexpr (ONE)
                    lds_st(base + (L1 + L1 / 16) * q + c, v[4 * q + c]);
                else
                    base[(L1 + L1 / 16) * q + c] = v[4 * q + c];
            }
    }

    // pass 1: butterfly i of the lane works in block b = NB1 (tl / 16) + i with s = tl % 16:
    // elements b L1 + s + 16 m, m < R1; register slots v[R1 i + m].  (This block assignment keeps
    // the two 16-lane halves of an N = 512 team on different banks.)
    static constexpr int STEP1 = L1 + L1 / 16; // physical distance between blocks
    static PSDK_HD int base1(int tl)
    {
        return STEP1 * NB1 * (tl >> 4) + (tl & 15); // + STEP1 i + 17 m
    }
    static PSDK_HD void load1(int tl, cf *v, const cf *frame)
    {
        const cf *base = frame + base1(tl);
#pragma unroll
        for (int i = 0; i < NB1; ++i)
#pragma unroll
            for (int m = 0; m < R1; ++m)
                v[R1 * i + m] = lds_ld(base + STEP1 * i + 17 * m);
    }
    static PSDK_HD void pass1(int tl, cf *v, const cf *tw1)
    {
        const int s = tl & 15;
#if PSDK_TW_ROWS
        if constexpr (NB1 == 1) { // (measured per size: see twiddle_rows in fft_core.h)
            Dft<R1>::run(v);
            twiddle_rows<R1, 1>(v, tw1 + s);
            return;
        }
#endif
#pragma unroll
        for (int i = 0; i < NB1; ++i) {
            Dft<R1>::run(v + R1 * i);
#pragma unroll
            for (int q = 1; q < R1; ++q)
                // plain (not lds_ld) loads: kept single, the R1 - 1 twiddle reads ended up serialised
                // through one register pair -- a chain of LDS round trips; left to the compiler they pair
                // up as ds_read2_b64 (dearer per byte) but are all in flight together: +2.5 % at N = 1024,
                // +13 % at N = 256
                v[R1 * i + q] = cmul(v[R1 * i + q], tw1[(q - 1) * 16 + s]);
        }
    }
    static PSDK_HD void store1(int tl, const cf *v, cf *frame)
    {
        cf *base = frame + base1(tl);
#pragma unroll
        for (int i = 0; i < NB1; ++i)
#pragma unroll
            for (int q = 0; q < R1; ++q)
                base[STEP1 * i + 17 * q] = v[R1 * i + q];
    }

    // pass 2: 16 consecutive elements per lane
    static PSDK_HD void load2(int tl, cf *v, const cf *frame)
    {
        const cf *base = frame + 17 * tl; // swz(16 tl + m) = 17 tl + m
#pragma unroll
        for (int m = 0; m < 16; ++m)
            v[m] = lds_ld(base + m);
    }
    static PSDK_HD void pass2(cf *v) { Dft<16>::run(v); }

    // ---- second exchange as planes (PLANES: N = 1024, the team is the wavefront) ----
    // Writer lane tl = 16 b + s stores slot q as two floats at dword row(q) + tl of the re
    // plane and of the im plane PLANE_IM dwords further on; reader t = 16 b + q finds its
    // sixteen re values in the sixteen consecutive dwords from row(q) + 16 b, and the im
    // values likewise.  "Constant + lane" is the address form of ds_write_addtid_b32.
    //
    // Row starts: a ds_read_b128 is served in the lane groups {0-3, 12-15, 20-27},
    // {4-11, 16-19, 28-31} and the same + 32, bank = dword mod 64, so the sixteen lanes of
    // a group must start in sixteen different bank quads.  With a(q) = (row(q) / 4) mod 16
    // a lane's quad is a(q) + 4 b + j (j: which of its four reads), and the groups ask that
    // a maps Q1 = {0-3, 12-15} one-to-one onto a set X with X + 8 = X and Q2 = {4-11} onto
    // (Z16 \ X) - 4.  X = {0-3, 8-11}: both halves land on X, each a twice; the sixteen rows
    // lie in memory in order of a, row k at dword 64 k + 4 a, which keeps them apart (a
    // never falls from a row to the next) and 16-byte aligned.  With l = q % 4, h = q / 4:
    // a = l + 8 (h / 2), k = 2 (l + 4 (h / 2)) + [q in Q2].  A plane ends at dword 1068 and
    // the im plane starts at FRAME (= 0 mod 64: the same banks), so the exchange stays
    // inside the frame.  tests/host/fft_planes_check.cpp counts it all.
    static constexpr bool PLANES = PSDK_ADDTID != 0 && TEAM == 64;
    static constexpr int PLANE_IM = FRAME; // dwords
    static constexpr PSDK_HD int plane_row(int q)
    {
        const int l = q & 3, hh = q >> 3, q2 = ((q >> 2) ^ (q >> 3)) & 1;
        return 4 * (33 * l + 136 * hh + 16 * q2); // 64 k + 4 a
    }
    static constexpr int PLANE_END = plane_row(11) + 64; // the last row in memory: l = 3, h = 2
    static_assert(!PLANES || (PLANE_END <= PLANE_IM && PLANE_IM + PLANE_END <= 2 * FRAME && PLANE_IM % 64 == 0),
                  "the planes stay inside the team frame, on the same banks");

    // M0 for the add-tid stores of a wavefront: the LDS byte address of its frame.  The
    // instruction takes M0[15:0] only, so a frame must START below 64 KiB (it may end above:
    // the offset and the lane are added to the 16-bit base, not wrapped); the kernel checks
    // its last frame against M0_LIMIT once, when it starts.
    static constexpr unsigned M0_LIMIT = 0x10000u;
    static PSDK_HD unsigned lds_base(const cf *frame)
    {
#if defined(__HIP_DEVICE_COMPILE__)
        return __builtin_amdgcn_readfirstlane(
            (unsigned)(uintptr_t)(const __attribute__((address_space(3))) void *)frame);
#else
        (void)frame;
        return 0;
#endif
    }
#if defined(__HIP_DEVICE_COMPILE__)
    // slots Q0 .. Q0 + 3.  M0 is compiler-reserved and not an operand a statement can
    // declare: the block saves it, sets it and puts it back, so it holds whether or not
    // the compiler keeps a value of its own there.  (Four slots a block: a statement takes
    // 30 operands at most, and 32 stores would need 66.)  The stores are not in the
    // compiler's lgkmcnt book-keeping; they need not be: the DS operations of a wavefront
    // complete in order, so a counted wait for a later read covers every store before it.
    template <int Q0>
    static __device__ __forceinline__ void store1_rows(unsigned m0, const cf *v)
    {
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\t"
                     "s_mov_b32 m0, %1\n\t"
                     "s_nop 0\n\t" // (SALU write of M0 -> add-tid DS operation: one wait state)
                     "ds_write_addtid_b32 %2 offset:%10\n\t"
                     "ds_write_addtid_b32 %3 offset:%11\n\t"
                     "ds_write_addtid_b32 %4 offset:%12\n\t"
                     "ds_write_addtid_b32 %5 offset:%13\n\t"
                     "ds_write_addtid_b32 %6 offset:%14\n\t"
                     "ds_write_addtid_b32 %7 offset:%15\n\t"
                     "ds_write_addtid_b32 %8 offset:%16\n\t"
                     "ds_write_addtid_b32 %9 offset:%17\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "s"(m0), "v"(v[Q0].re), "v"(v[Q0].im), "v"(v[Q0 + 1].re), "v"(v[Q0 + 1].im),
                       "v"(v[Q0 + 2].re), "v"(v[Q0 + 2].im), "v"(v[Q0 + 3].re), "v"(v[Q0 + 3].im),
                       "n"(4 * plane_row(Q0)), "n"(4 * (PLANE_IM + plane_row(Q0))),
                       "n"(4 * plane_row(Q0 + 1)), "n"(4 * (PLANE_IM + plane_row(Q0 + 1))),
                       "n"(4 * plane_row(Q0 + 2)), "n"(4 * (PLANE_IM + plane_row(Q0 + 2))),
                       "n"(4 * plane_row(Q0 + 3)), "n"(4 * (PLANE_IM + plane_row(Q0 + 3)))
                     : "memory");
    }
#endif
    // 32 ds_write_addtid_b32 (2 store-path cycles each) in place of store1's 16 8-byte stores
    static PSDK_HD void store1_planes(int tl, const cf *v, cf *frame, unsigned m0)
    {
#if defined(__HIP_DEVICE_COMPILE__)
        (void)tl, (void)frame;
        store1_rows<0>(m0, v);
        store1_rows<4>(m0, v);
        store1_rows<8>(m0, v);
        store1_rows<12>(m0, v);
#else
        (void)m0;
        float *f = reinterpret_cast<float *>(frame);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            f[plane_row(q) + tl] = v[q].re;
            f[PLANE_IM + plane_row(q) + tl] = v[q].im;
        }
#endif
    }
    // dword of the reader's m = 0
    static PSDK_HD int plane_base(int tl) { return plane_row(tl & 15) + 16 * (tl >> 4); }
    // 4 + 4 ds_read_b128 (4 LDS cycles each) where load2 issues 16 ds_read_b64 (2 each)
    static PSDK_HD void load2_planes(int tl, cf *v, const cf *frame)
    {
        const float *f = reinterpret_cast<const float *>(frame) + plane_base(tl);
#if defined(__HIP_DEVICE_COMPILE__)
        typedef float f4v __attribute__((ext_vector_type(4)));
        typedef const volatile __attribute__((address_space(3))) f4v *lds_f4v;
        const lds_f4v p = (lds_f4v)f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f4v re = p[j], im = p[PLANE_IM / 4 + j];
            v[4 * j] = {re.x, im.x};
            v[4 * j + 1] = {re.y, im.y};
            v[4 * j + 2] = {re.z, im.z};
            v[4 * j + 3] = {re.w, im.w};
        }
#else
#pragma unroll
        for (int m = 0; m < 16; ++m)
            v[m] = {f[m], f[PLANE_IM + m]};
#endif
    }
};

} // namespace psdk
