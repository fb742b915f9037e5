// Host side of the converter of stabilizer-stream_amd/csrc/sample_int.h (sint_cvt_thread, the thread function of
// sample_cvt_int_kernel: the integer feeds of the PSD, pair and matrix objects, psdc_sint_*) -- the same source the device runs.
//   sample_cvt_emul            runs every check below and prints one line a part; exit status 0 if all hold
//     values   every int16 and every int8 value, three scales, at every position of a group (wide and element-wise loads) and in
//              the head and the tail of a launch, against (float)v * scale bit for bit
//     launch   sint_cvt_thread run for every thread of a launch (x: the grid's threads, y: the channel): nch 1 ... 4, every
//              destination phase, source misalignments 0 ... 7 integers that differ from channel to channel (so the per-channel
//              bit of the mask matters), lengths 0 ... 40 and around one block of groups.  Sources and destinations are heap
//              buffers of the exact size; the destinations sit between guard words inside theirs.  Every output equals
//              (float)v * scale to the bit, every destination element is written exactly once, every guard word is intact.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -I<csrc> sample_cvt_emul.cpp, and once more with -fsanitize=address,undefined
// (tests/test_int_feed_real_host.py does both).
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

static const float SCALES[3] = {0x1p-15f, 1.0f, 3.0e-3f};
static const uint32_t UNWRITTEN = 0x7FC5A5A5u, GUARD = 0x7FCBEEF1u; // NaN payloads no conversion produces
constexpr int GUARDS = 4;                                           // guard words on each side of a destination

// a buffer of the exact size, so that the address sanitizer sees a byte read or written outside it
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

// One launch.  Channel c's source starts src_off[c] integers into its buffer (which ends with its last integer); every destination
// starts `lead` floats in front of a 16-byte boundary, behind GUARDS guard words, and is followed by GUARDS more.  fill(c, i) gives
// the integers.  Runs the whole grid: every thread of every block, every channel up to 4 so that ch >= nch is seen to do nothing.
template <typename T, typename Fill>
static void launch(unsigned nch, unsigned lead, const unsigned (&src_off)[4], unsigned long long len, float scale, Fill fill,
                   unsigned long long &outputs)
{
    const size_t pad = 4 + ((4 - lead) & 3); // floats in front of the destination: GUARDS of them are guards (the base is 64-byte aligned)
    std::vector<Exact *> sb, db;
    SintCvtJob job{};
    job.nch = nch;
    job.len = len;
    job.scale = scale;
    for (unsigned c = 0; c < nch; ++c) {
        sb.push_back(new Exact((src_off[c] + len) * sizeof(T)));
        db.push_back(new Exact((pad + len + GUARDS) * sizeof(float)));
        T *s = (T *)sb[c]->base + src_off[c];
        for (unsigned long long i = 0; i < len; ++i)
            s[i] = fill(c, i);
        uint32_t *d = (uint32_t *)db[c]->base;
        for (size_t k = 0; k < pad + len + GUARDS; ++k)
            d[k] = k >= pad && k < pad + len ? UNWRITTEN : GUARD;
        job.src[c] = s;
        job.dst[c] = (float *)db[c]->base + pad;
    }
    for (unsigned c = 1; c < nch; ++c)
        CHECK((((uintptr_t)job.dst[0] ^ (uintptr_t)job.dst[c]) & 15) == 0, "the destinations do not share their phase");
    const unsigned head = sint_head(job.dst[0], len);
    CHECK(head == (lead < len ? lead : (unsigned)len), "head %u lead %u len %llu", head, lead, len);
    int mask = 0;
    for (unsigned c = 0; c < nch; ++c)
        mask |= (sint_src_aligned(job.src[c], head, sizeof(T)) ? 1 : 0) << c;
    const unsigned long long threads = sint_threads(head, len), grid = (threads + SINT_BLOCK - 1) / SINT_BLOCK * SINT_BLOCK;
    // Twice, the threads in ascending and in descending order: a thread must find the elements of its own span unwritten and
    // leave them written, so an element that two threads write, or that a thread outside its span writes, shows in one of the
    // two orders; channels past nch have null pointers and must do nothing
    std::vector<std::vector<unsigned char>> wrote(nch, std::vector<unsigned char>(len, 0));
    for (int order = 0; order < 2; ++order) {
        for (unsigned c = 0; c < nch; ++c)
            for (unsigned long long i = 0; i < len; ++i)
                memcpy(job.dst[c] + i, &UNWRITTEN, 4);
        for (unsigned long long t = 0; t < 4 * grid; ++t) {
            const unsigned long long u = order ? 4 * grid - 1 - t : t;
            const unsigned ch = (unsigned)(u / grid);
            const unsigned long long g = u % grid;
            const SintSpan sp = ch < nch ? sint_span(g, head, len, (mask >> ch) & 1) : SintSpan{0, 0, false};
            if (g >= threads)
                CHECK(sp.count == 0, "a thread past the last group has work: g %llu", g);
            for (unsigned long long i = sp.first; i < sp.first + sp.count; ++i) {
                uint32_t w;
                memcpy(&w, job.dst[ch] + i, 4);
                CHECK(w == UNWRITTEN, "element %llu of channel %u is written by another thread than %llu", i, ch, g);
            }
            sint_cvt_thread<T>(job, head, mask, ch, g);
            for (unsigned long long i = sp.first; i < sp.first + sp.count; ++i) {
                uint32_t w;
                memcpy(&w, job.dst[ch] + i, 4);
                if (w != UNWRITTEN && order == 0)
                    ++wrote[ch][i];
            }
        }
    }
    for (unsigned c = 0; c < nch; ++c) {
        const T *s = (const T *)job.src[c];
        const uint32_t *d = (const uint32_t *)db[c]->base;
        for (size_t k = 0; k < pad; ++k)
            CHECK(d[k] == GUARD, "guard word %zu in front of channel %u is overwritten (len %llu lead %u)", k, c, len, lead);
        for (size_t k = pad + len; k < pad + len + GUARDS; ++k)
            CHECK(d[k] == GUARD, "guard word %zu behind channel %u is overwritten (len %llu lead %u)", (size_t)(k - pad - len), c, len, lead);
        for (unsigned long long i = 0; i < len; ++i) {
            CHECK(wrote[c][i] == 1, "element %llu of channel %u written %d times (len %llu head %u off %u)", i, c, wrote[c][i], len,
                  head, src_off[c]);
            CHECK(same_bits(job.dst[c][i], want((int)s[i], scale)), "channel %u element %llu: v %d scale %a got %a (len %llu head %u off %u)",
                  c, i, (int)s[i], (double)scale, (double)job.dst[c][i], len, head, src_off[c]);
            ++outputs;
        }
    }
    for (Exact *e : sb)
        delete e;
    for (Exact *e : db)
        delete e;
}

// every value of the type at every position of a launch: blocks of all values in order, shifted by the channel, through a launch
// whose channels are read wide (aligned source) and element-wise (misaligned), with a head and a partial tail
template <typename T>
static void values_kind(const char *name)
{
    const long lo = sizeof(T) == 2 ? -32768 : -128, span = sizeof(T) == 2 ? 65536 : 256;
    unsigned long long n = 0;
    for (float scale : SCALES)
        for (unsigned lead = 0; lead < 4; ++lead) {
            // 4 passes of every value, shifted by one position a pass: every value meets every position of a group; + 7: a partial tail
            const unsigned long long len = 4ull * span + 7;
            const unsigned off[4] = {(4 - lead) & 3, ((4 - lead) & 3) + 1, 2, 7}; // channel 0 wide, the others as they fall
            launch<T>(2, lead, off, len, scale, [&](unsigned c, unsigned long long i) { return (T)(lo + (long)((i + i / span + c) % span)); }, n);
        }
    printf("values %s: %llu conversions checked\n", name, n);
}

static std::vector<unsigned long long> lengths()
{
    std::vector<unsigned long long> v;
    for (unsigned long long l = 0; l <= 40; ++l)
        v.push_back(l);
    for (unsigned long long l = SINT_BLOCK * SINT_Q - 5; l <= SINT_BLOCK * SINT_Q + 6; ++l) // around one block of groups
        v.push_back(l);
    return v;
}

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

template <typename T>
static void launch_kind(const char *name)
{
    unsigned long long launches = 0, n = 0;
    for (float scale : SCALES)
        for (unsigned nch = 1; nch <= 4; ++nch)
            for (unsigned lead = 0; lead < 4; ++lead)
                for (unsigned mis = 0; mis < 8; ++mis) // channel c's source is (mis + 3 c) mod 8 integers past a 64-byte boundary
                    for (unsigned long long len : lengths()) {
                        const unsigned off[4] = {mis, (mis + 3) & 7, (mis + 6) & 7, (mis + 9) & 7};
                        launch<T>(nch, lead, off, len, scale, [&](unsigned c, unsigned long long i) { return sample<T>(i + 5 * c + mis); }, n);
                        ++launches;
                    }
    printf("launch %s: %llu launches, %llu outputs equal to (float)v * scale bit for bit, each written once, guards intact\n", name,
           launches, n);
}

int main()
{
    values_kind<int16_t>("s16");
    values_kind<int8_t>("s8");
    launch_kind<int16_t>("s16");
    launch_kind<int8_t>("s8");
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("sample_cvt: all checks hold\n");
    return 0;
}
