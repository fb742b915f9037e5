// Host side of stabilizer-stream_amd/csrc/sample_int.h, the integer sample feeds (the same source the device runs).
//   sample_int_emul            runs every check below and prints one line a check; exit status 0 if all hold
//     unpack   sint_lane, SintGroup::get behind sint_load_group, sint_load1 and sint_load1c: every int16 and every int8 value in every
//              lane position of the packed words, three scales, against (float)v * scale bit for bit
//     map      sint_span: every kind, head, source misalignment and length -- every unit read once, every destination element
//              written once, no byte outside the source, a wide load only where its address is aligned
//     mix      sint_zoom_thread / sint_iq_thread / sint_iq_pair_thread run for every thread of a launch on buffers of the exact size,
//              against zoom_mix / iq_mix of zoom_lo.h / iq_lo.h fed the converted f32 samples: equal bits, without and with a
//              carrier, and with shared and distinct carriers on a pair
// Build: g++ -O2 -std=c++17 -ffp-contract=off -I<csrc> sample_int_emul.cpp, and once more with -fsanitize=address,undefined
// (tests/test_int_feed_host.py does both).
#include "sample_int.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace psdk;

static int failures = 0;
#define CHECK(cond, ...)                                                                                                \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            if (++failures <= 20) {                                                                                    \
                fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond);                                        \
                fprintf(stderr, __VA_ARGS__);                                                                          \
                fprintf(stderr, "\n");                                                                                 \
            }                                                                                                          \
        }                                                                                                              \
    } while (0)

static bool same_bits(float a, float b) { return memcmp(&a, &b, sizeof a) == 0; }

// the rule, spelled apart from the header: the conversion, then one product
static float want(int v, float scale)
{
    volatile float f = (float)v;
    volatile float p = f * scale;
    return p;
}

static uint32_t rng_state = 0x2545F491u;
static uint32_t rng()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}

static const float SCALES[3] = {0x1p-15f, 1.0f, 3.0517578e-5f * 1.2345678f};

// ---- unpack ------------------------------------------------------------------------------------------------------------
template <typename T, int C>
static void unpack_group(long lo, long hi, unsigned long long &n)
{
    using G = SintGroup<T, C>;
    alignas(16) T buf[SINT_Q * C];
    for (float scale : SCALES)
        for (long v = lo; v <= hi; ++v)
            for (int e = 0; e < SINT_Q * C; ++e) { // v at element e of the group, the other lanes filled with other bits
                const uint32_t fill = rng();
                for (int k = 0; k < SINT_Q * C; ++k)
                    buf[k] = (T)(fill >> (k % 3)) ^ (T)(k & 1 ? -1 : 0);
                buf[e] = (T)v;
                G g;
                sint_load_group<T, C>(buf, g);
                const float got = g.get(e / C, e % C, scale);
                CHECK(same_bits(got, want((int)v, scale)), "group<%d,%d> v=%ld e=%d scale=%a got %a", (int)sizeof(T), C, v, e,
                      (double)scale, (double)got);
                ++n;
            }
}

template <typename T>
static void unpack_kind(const char *name)
{
    const long lo = sizeof(T) == 2 ? -32768 : -128, hi = sizeof(T) == 2 ? 32767 : 127;
    constexpr int LANES = 4 / (int)sizeof(T), B = 8 * (int)sizeof(T);
    unsigned long long n = 0;
    for (float scale : SCALES)
        for (long v = lo; v <= hi; ++v) {
            for (int lane = 0; lane < LANES; ++lane) { // the word itself, every lane, zeros and ones and noise around it
                const uint32_t mask = (B == 32 ? 0xFFFFFFFFu : ((1u << B) - 1u)) << (B * lane);
                for (uint32_t around : {0u, 0xFFFFFFFFu, rng()}) {
                    const uint32_t w = (around & ~mask) | (((uint32_t)v << (B * lane)) & mask);
                    const float got = sint_lane<T>(w, lane, scale);
                    CHECK(same_bits(got, want((int)v, scale)), "%s lane v=%ld lane=%d w=%08x got %a", name, v, lane, w, (double)got);
                    ++n;
                }
            }
            const T one = (T)v;
            CHECK(same_bits(sint_load1(&one, scale), want((int)v, scale)), "%s load1 v=%ld", name, v);
            for (int c = 0; c < 2; ++c) { // a (re, im) unit read at its own size
                alignas(4) T pr[2] = {(T)rng(), (T)rng()};
                pr[c] = (T)v;
                float re, im;
                sint_load1c(pr, scale, re, im);
                CHECK(same_bits(c ? im : re, want((int)v, scale)) && same_bits(c ? re : im, want((int)pr[1 - c], scale)),
                      "%s load1c v=%ld c=%d", name, v, c);
                n += 2;
            }
        }
    unpack_group<T, 1>(lo, hi, n);
    unpack_group<T, 2>(lo, hi, n);
    printf("unpack %s: %llu conversions checked\n", name, n);
}

// ---- index map ---------------------------------------------------------------------------------------------------------
static std::vector<unsigned long long> lengths()
{
    std::vector<unsigned long long> v;
    for (unsigned long long l = 0; l <= 70; ++l)
        v.push_back(l);
    for (unsigned long long l = SINT_BLOCK * SINT_Q - 6; l <= SINT_BLOCK * SINT_Q + 9; ++l) // around one block of groups
        v.push_back(l);
    v.push_back(2 * SINT_BLOCK * SINT_Q + 3);
    return v;
}

static void map_check()
{
    unsigned long long cases = 0;
    alignas(64) static unsigned char srcbuf[64 + 4 * 4 * (2 * SINT_BLOCK * SINT_Q + 16)];
    alignas(64) static float dstbuf[2 * SINT_BLOCK * SINT_Q + 32];
    for (int kind : {SAMPLE_S16, SAMPLE_S8})
        for (int comps = 1; comps <= 2; ++comps) {
            const size_t unit = (size_t)sint_bytes(kind) * comps;
            for (unsigned lead = 0; lead < 4; ++lead)
                for (unsigned off = 0; off < 4; ++off) // the source's misalignment class: units past a group boundary
                    for (unsigned long long len : lengths()) {
                        const unsigned char *src = srcbuf + off * unit;
                        const float *dst = dstbuf + ((4 - lead) & 3);
                        const unsigned head = sint_head(dst, len);
                        CHECK(head == (lead < len ? lead : (unsigned)len), "head %u lead %u len %llu", head, lead, len);
                        const bool al = sint_src_aligned(src, head, unit);
                        CHECK(al == (((off + head) & 3) == 0), "aligned flag off %u head %u", off, head);
                        std::vector<unsigned char> read(len, 0), wrote(len, 0);
                        const unsigned long long threads = sint_threads(head, len);
                        const unsigned long long grid = (threads + SINT_BLOCK - 1) / SINT_BLOCK * SINT_BLOCK;
                        for (unsigned long long g = 0; g < grid; ++g) {
                            const SintSpan sp = sint_span(g, head, len, al);
                            CHECK(sp.count <= (unsigned)SINT_Q, "count %u", sp.count);
                            if (g >= threads)
                                CHECK(sp.count == 0, "a thread past the last group has work: g %llu", g);
                            if (!sp.count)
                                continue;
                            const unsigned long long b0 = sp.first * unit, b1 = (sp.first + sp.count) * unit; // the bytes it reads
                            CHECK(b1 <= len * unit && b0 < b1, "bytes [%llu, %llu) leave the source of %llu", b0, b1,
                                  (unsigned long long)(len * unit));
                            if (sp.wide) {
                                CHECK(sp.count == (unsigned)SINT_Q, "a wide load of a partial group");
                                CHECK((uintptr_t)(src + b0) % (SINT_Q * unit) == 0, "a wide load at a misaligned address");
                            }
                            if (g != 0) // a group's destination is a 16-byte store where it is full
                                CHECK(sp.count < (unsigned)SINT_Q || (uintptr_t)(dst + sp.first) % 16 == 0, "a misaligned 16-byte store");
                            for (unsigned long long i = sp.first; i < sp.first + sp.count && i < len; ++i)
                                ++read[i], ++wrote[i];
                        }
                        for (unsigned long long i = 0; i < len; ++i)
                            CHECK(read[i] == 1 && wrote[i] == 1, "unit %llu read %d written %d times (len %llu head %u)", i, read[i],
                                  wrote[i], len, head);
                        ++cases;
                    }
        }
    printf("map: %llu launches checked\n", cases);
}

// ---- mixer parity ------------------------------------------------------------------------------------------------------
// buffers of the exact size, so that the address sanitizer sees a byte read or written outside them
struct Exact {
    void *base = nullptr;
    explicit Exact(size_t bytes)
    {
        if (posix_memalign(&base, 64, bytes ? bytes : 1))
            abort();
        memset(base, 0x5A, bytes ? bytes : 1);
    }
    ~Exact() { free(base); }
    Exact(const Exact &) = delete;
};

template <typename T>
static T sample(unsigned long long i)
{
    const long lo = sizeof(T) == 2 ? -32768 : -128, hi = sizeof(T) == 2 ? 32767 : 127;
    switch (i % 11) {
    case 0: return (T)lo;
    case 3: return (T)hi;
    case 5: return (T)0;
    case 7: return (T)-1;
    default: return (T)rng();
    }
}

struct Carrier {
    unsigned long long ftw[2], phase0[2];
    const char *name;
};
static const Carrier CARRIERS[] = {
    {{0, 0}, {0, 0}, "none"},
    {{0x3C6EF372FE94F82Bull, 0x3C6EF372FE94F82Bull}, {0x9E3779B97F4A7C15ull, 0x9E3779B97F4A7C15ull}, "shared"},
    {{0x3C6EF372FE94F82Bull, 0xC2B2AE3D27D4EB4Full}, {0x9E3779B97F4A7C15ull, 0x165667B19E3779F9ull}, "distinct"},
    {{0x3C6EF372FE94F82Bull, 0x3C6EF372FE94F82Bull}, {0x9E3779B97F4A7C15ull, 0x165667B19E3779F9ull}, "equal ftw, distinct phase"},
};

template <typename T>
static void mix_kind(const char *name)
{
    unsigned long long launches = 0;
    const float scale = SCALES[2];
    const unsigned long long j0 = 0x1234567ull;
    for (const Carrier &car : CARRIERS)
        for (unsigned lead = 0; lead < 4; ++lead)
            for (unsigned off = 0; off < 4; ++off)
                for (unsigned long long len : lengths()) {
                    const size_t pad = (4 - lead) & 3;
                    // --- real: zoom
                    {
                        Exact sb((off + len) * sizeof(T)), di((pad + len) * 4), dq((pad + len) * 4);
                        T *src = (T *)sb.base + off;
                        for (unsigned long long i = 0; i < len; ++i)
                            src[i] = sample<T>(i + off);
                        SintMixJob job{src, (float *)di.base + pad, (float *)dq.base + pad, len, j0, car.ftw[0], car.phase0[0], scale};
                        const unsigned head = sint_head(job.dst_i, len);
                        const bool al = sint_src_aligned(src, head, sizeof(T));
                        for (unsigned long long g = 0; g < sint_threads(head, len) + 3; ++g)
                            sint_zoom_thread<T>(job, head, al, g);
                        for (unsigned long long i = 0; i < len; ++i) {
                            float wi, wq;
                            zoom_mix(want(src[i], scale), car.phase0[0] + car.ftw[0] * (j0 + i), wi, wq);
                            CHECK(same_bits(job.dst_i[i], wi) && same_bits(job.dst_q[i], wq), "%s zoom %s len %llu head %u off %u i %llu",
                                  name, car.name, len, head, off, i);
                        }
                        ++launches;
                    }
                    // --- complex: iq, and both sides of a pair
                    {
                        Exact sa(2 * (off + len) * sizeof(T)), sb(2 * (off + len) * sizeof(T));
                        Exact d0((pad + len) * 4), d1((pad + len) * 4), d2((pad + len) * 4), d3((pad + len) * 4), e0((pad + len) * 4),
                            e1((pad + len) * 4);
                        T *za = (T *)sa.base + 2 * off, *zb = (T *)sb.base + 2 * off;
                        for (unsigned long long i = 0; i < 2 * len; ++i)
                            za[i] = sample<T>(i + off), zb[i] = sample<T>(i + 5 + off);
                        SintMixJob job{za, (float *)e0.base + pad, (float *)e1.base + pad, len, j0, car.ftw[0], car.phase0[0], scale};
                        SintPairMixJob pj{};
                        pj.src[0] = za, pj.src[1] = zb;
                        pj.dst[0] = (float *)d0.base + pad, pj.dst[1] = (float *)d1.base + pad;
                        pj.dst[2] = (float *)d2.base + pad, pj.dst[3] = (float *)d3.base + pad;
                        pj.len = len, pj.j0 = j0, pj.scale = scale;
                        for (int s = 0; s < 2; ++s)
                            pj.ftw[s] = car.ftw[s], pj.phase0[s] = car.phase0[s];
                        const unsigned head = sint_head(job.dst_i, len);
                        const bool ala = sint_src_aligned(za, head, 2 * sizeof(T)), alb = sint_src_aligned(zb, head, 2 * sizeof(T));
                        for (unsigned long long g = 0; g < sint_threads(head, len) + 3; ++g) {
                            sint_iq_thread<T>(job, head, ala, g);
                            // side b's flag set and cleared in turn: each side is judged on its own
                            sint_iq_pair_thread<T>(pj, head, (ala ? 1 : 0) | (alb && (len & 1) ? 2 : 0), g);
                        }
                        for (unsigned long long i = 0; i < len; ++i) {
                            float wi, wq, vi, vq;
                            iq_mix(want(za[2 * i], scale), want(za[2 * i + 1], scale), car.phase0[0] + car.ftw[0] * (j0 + i), wi, wq);
                            iq_mix(want(zb[2 * i], scale), want(zb[2 * i + 1], scale), car.phase0[1] + car.ftw[1] * (j0 + i), vi, vq);
                            CHECK(same_bits(job.dst_i[i], wi) && same_bits(job.dst_q[i], wq), "%s iq %s len %llu head %u off %u i %llu", name,
                                  car.name, len, head, off, i);
                            CHECK(same_bits(pj.dst[0][i], wi) && same_bits(pj.dst[1][i], wq) && same_bits(pj.dst[2][i], vi) &&
                                      same_bits(pj.dst[3][i], vq),
                                  "%s pair %s len %llu head %u off %u i %llu", name, car.name, len, head, off, i);
                        }
                        launches += 2;
                    }
                }
    printf("mix %s: %llu launches equal to the f32 mixers bit for bit\n", name, launches);
}

int main()
{
    unpack_kind<int16_t>("s16");
    unpack_kind<int8_t>("s8");
    map_check();
    mix_kind<int16_t>("s16");
    mix_kind<int8_t>("s8");
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("sample_int: all checks hold\n");
    return 0;
}
