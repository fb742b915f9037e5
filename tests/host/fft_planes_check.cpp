// Host check of the N = 1024 team FFT's second exchange as re / im planes (csrc/fft_team.h: store1_planes / load2_planes,
// the add-tid form of the kernel): the addressing is run lane by lane under the gfx950 LDS rules --
//   ds_write_addtid_b32: the 64 lanes of an instruction write 64 consecutive dwords from a constant,
//   ds_read_b128: lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32, one LDS cycle a group when its
//                 sixteen lanes touch 64 different banks, bank = (byte address / 4) mod 64, 16-byte aligned addresses --
// and must show ZERO bank conflicts, aligned reads, rows that do not overlap, an extent inside the team frame; and the
// |X|^2 of the transform through the planes must equal, bit for bit, the transform through the cf frame (store1 / load2).
// Build: g++ -O2 -std=c++17 -I<csrc>.
#include "fft_team.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>
using namespace psdk;

using T = TeamFft<1024>;
static_assert(T::PLANES, "built with PSDK_ADDTID=0: nothing to check");
static constexpr int TEAM = T::TEAM;
static constexpr int FRAME_DW = 2 * T::FRAME; // dwords of a team frame

static const int GROUPS[4][16] = {
    {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
    {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
    {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
    {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63},
};

static int check_layout()
{
    int bad = 0;
    // the frames of a workgroup are sizeof(cf) * FRAME bytes apart from a 16-byte aligned start
    if ((sizeof(cf) * T::FRAME) % 16 != 0) {
        printf("frame size %zu B is not a multiple of 16\n", sizeof(cf) * T::FRAME);
        bad = 1;
    }
    // stores: instruction (q, plane) writes dword plane + plane_row(q) + lane; every dword of the exchange exactly once
    std::vector<int> owner(FRAME_DW, -1);
    int hi = 0;
    for (int plane = 0; plane < 2; ++plane)
        for (int q = 0; q < 16; ++q) {
            const int row = plane * T::PLANE_IM + T::plane_row(q);
            if (row < 0 || row + 64 > FRAME_DW) {
                printf("row q=%d plane=%d: dwords [%d, %d) leave the frame of %d\n", q, plane, row, row + 64, FRAME_DW);
                return 1;
            }
            if (4 * row > 0xFFFF) {
                printf("row q=%d plane=%d: byte offset %d does not fit the 16-bit DS offset field\n", q, plane, 4 * row);
                bad = 1;
            }
            std::set<int> banks; // 2 x 32 lanes, bank = dword mod 32: consecutive dwords, checked all the same
            for (int lane = 0; lane < 64; ++lane) {
                const int dw = row + lane;
                if (owner[dw] >= 0) {
                    printf("rows overlap: dword %d written by instruction %d and by q=%d plane=%d\n", dw, owner[dw], q, plane);
                    bad = 1;
                }
                owner[dw] = plane * 16 + q;
                if (lane < 32)
                    banks.insert(dw % 32);
            }
            if (banks.size() != 32) {
                printf("store q=%d plane=%d: bank conflict\n", q, plane);
                bad = 1;
            }
            hi = std::max(hi, row + 64);
        }
    // reads: lane t issues, for plane p and j < 4, a 16-byte read at dword p PLANE_IM + plane_base(t) + 4 j
    long cycles = 0, ideal = 0;
    for (int plane = 0; plane < 2; ++plane)
        for (int j = 0; j < 4; ++j) {
            for (int g = 0; g < 4; ++g) {
                std::vector<std::set<int>> per(64); // distinct dword addresses per bank
                for (int i = 0; i < 16; ++i) {
                    const int t = GROUPS[g][i];
                    const int dw = plane * T::PLANE_IM + T::plane_base(t) + 4 * j;
                    if ((4 * dw) % 16 != 0) {
                        printf("read lane %d plane %d j %d: byte address %d is not 16-byte aligned\n", t, plane, j, 4 * dw);
                        bad = 1;
                    }
                    for (int e = 0; e < 4; ++e)
                        per[(dw + e) % 64].insert(dw + e);
                }
                size_t worst = 1;
                for (auto &s : per)
                    worst = std::max(worst, s.size());
                cycles += (long)worst, ++ideal;
            }
        } // (that a reader finds its writer's dwords is what the bit-for-bit comparison below carries)
    printf("planes: 32 stores of 64 consecutive dwords, extent %d of %d dwords; 8 ds_read_b128: %ld LDS cycles (ideal %ld)\n", hi,
           FRAME_DW, cycles, ideal);
    if (cycles != ideal) {
        printf("ds_read_b128 bank conflicts: %ld extra cycles\n", cycles - ideal);
        bad = 1;
    }
    if (hi > FRAME_DW)
        bad = 1;
    return bad;
}

// the transform of one seeded input through either second exchange; |X|^2 per bin
static void transform(unsigned seed, bool planes, std::vector<float> &pw)
{
    std::vector<cf> z(1024), frame(T::FRAME), tw0(T::TW0_SIZE), tw1(T::TW1_SIZE);
    srand(seed);
    for (auto &x : z) {
        x.re = (float)rand() / RAND_MAX - 0.5f;
        x.im = (float)rand() / RAND_MAX - 0.5f;
    }
    for (int c = 0; c < 4; ++c)
        for (int tl = 0; tl < TEAM; ++tl) {
            const double a = -2.0 * M_PI * (double)(4 * tl + c) / 1024.0;
            tw0[c * TEAM + tl] = {(float)cos(a), (float)sin(a)};
        }
    for (int q = 1; q < T::R1; ++q)
        for (int s = 0; s < 16; ++s) {
            const double a = -2.0 * M_PI * (double)(s * q) / (double)T::L1;
            tw1[(q - 1) * 16 + s] = {(float)cos(a), (float)sin(a)};
        }
    std::vector<std::vector<cf>> regs(TEAM, std::vector<cf>(16));
    for (int t = 0; t < TEAM; ++t)
        for (int m = 0; m < 4; ++m)
            for (int c = 0; c < 4; ++c)
                regs[t][4 * m + c] = z[4 * t + c + 256 * m];
    // (a wavefront runs in lockstep: every lane's load1 is done before any lane's second-exchange store)
    for (int t = 0; t < TEAM; ++t) T::pass0(t, regs[t].data(), tw0.data());
    for (int t = 0; t < TEAM; ++t) T::store0(t, regs[t].data(), frame.data());
    for (int t = 0; t < TEAM; ++t) T::load1(t, regs[t].data(), frame.data());
    for (int t = 0; t < TEAM; ++t) T::pass1(t, regs[t].data(), tw1.data());
    if (planes) {
        for (int t = 0; t < TEAM; ++t) T::store1_planes(t, regs[t].data(), frame.data(), 0u);
        for (int t = 0; t < TEAM; ++t) T::load2_planes(t, regs[t].data(), frame.data());
    } else {
        for (int t = 0; t < TEAM; ++t) T::store1(t, regs[t].data(), frame.data());
        for (int t = 0; t < TEAM; ++t) T::load2(t, regs[t].data(), frame.data());
    }
    for (int t = 0; t < TEAM; ++t) T::pass2(regs[t].data());
    pw.assign(1024, -1.0f);
    for (int t = 0; t < TEAM; ++t)
        for (int q = 0; q < 16; ++q) {
            const cf x = regs[t][q];
            pw[T::freq_of(t, q)] = x.re * x.re + x.im * x.im;
        }
}

int main()
{
    int bad = check_layout();
    for (unsigned seed = 1; seed <= 8; ++seed) {
        std::vector<float> a, b;
        transform(1000 + seed, false, a);
        transform(1000 + seed, true, b);
        double sum = 0;
        for (float x : a)
            sum += x;
        const bool same = memcmp(a.data(), b.data(), sizeof(float) * 1024) == 0;
        printf("seed %u: sum |X|^2 = %.6g, planes %s the cf frame\n", seed, sum, same ? "bit-identical to" : "DIFFER from");
        if (!same || !(sum > 0))
            bad = 1;
    }
    printf(bad ? "FAIL\n" : "OK\n");
    return bad;
}
