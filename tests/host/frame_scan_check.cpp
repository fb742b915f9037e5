// tests/host/frame_scan_check.cpp -- the frame-header scanner of every frames call (stabilizer-stream_amd/csrc/frame_scan.h) on the
// CPU, driven as its callers drive it: run by run (run_start), piece by piece (scan_piece), Loss committed with each piece.
// TEST INFRASTRUCTURE; tests/test_frame_scan_host.py writes the blobs and compares the lines with a frame-by-frame walk.
//
// usage: frame_scan_check FILE [gathered]
// FILE holds one or more blobs: four little-endian u64 (frame_size, n_frames, the piece limit in frames, 1 for the AdcDac-only
// rule) and n_frames * frame_size frame bytes.  `gathered` scans a copy of the headers alone, 8 bytes a frame, as the calls for
// frames in device memory do; without it the headers are read where they are, frame_size bytes apart.
// One line per blob: the return code, frames accepted, Loss received / dropped / next_seq / have_seq, and "id:frames" of every run
// that took a frame.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "frame_scan.h"

using namespace psdrt;

namespace {

std::string scan_call(const uint8_t *frames, size_t frame_size, size_t n_frames, size_t piece, bool adcdac_only, bool gathered)
{
    size_t good = 0;
    psdc_loss loss{};
    std::string runs;
    bool go = false;
    int bad = check_frames_call(frames, frame_size, n_frames, &go);
    if (go) {
        std::vector<uint8_t> hdr8;
        for (size_t f = 0; gathered && f < n_frames; ++f)
            hdr8.insert(hdr8.end(), frames + f * frame_size, frames + f * frame_size + 8);
        const HdrView hdr = gathered ? HdrView{hdr8.data(), 8} : HdrView{frames, frame_size};
        const size_t payload = frame_size - 8;
        size_t f0 = 0;
        while (f0 < n_frames && bad == PSDC_OK) {
            const WireFmt *wf = nullptr;
            bad = run_start(hdr, f0, adcdac_only, &wf);
            if (bad != PSDC_OK)
                break;
            size_t in_run = 0;
            int stop = SCAN_LIMIT;
            while (f0 < n_frames && stop == SCAN_LIMIT) {
                psdc_loss trial = loss;
                const size_t cnt = scan_piece(hdr, *wf, payload, f0, std::min(piece, n_frames - f0), adcdac_only, &trial, &stop);
                if (cnt == 0)
                    break;
                loss = trial; // (a caller enqueues the piece's samples here)
                good += cnt;
                in_run += cnt;
                f0 += cnt;
            }
            if (stop < 0)
                bad = stop;
            if (in_run)
                runs += " " + std::to_string(wf->id) + ":" + std::to_string(in_run);
        }
    }
    char line[160];
    snprintf(line, sizeof line, "%d %zu %llu %llu %u %u", bad, good, (unsigned long long)loss.received,
             (unsigned long long)loss.dropped, loss.next_seq, loss.have_seq);
    return line + runs;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 2 || (argc > 2 && strcmp(argv[2], "gathered") != 0)) {
        fprintf(stderr, "usage: frame_scan_check FILE [gathered]\n");
        return 2;
    }
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) {
        perror(argv[1]);
        return 2;
    }
    std::vector<uint8_t> data;
    uint8_t buf[1 << 16];
    for (size_t got; (got = fread(buf, 1, sizeof buf, fp)) > 0;)
        data.insert(data.end(), buf, buf + got);
    fclose(fp);
    size_t pos = 0;
    while (pos < data.size()) {
        uint64_t w[4];
        if (data.size() - pos < sizeof w) {
            fprintf(stderr, "truncated blob header at byte %zu\n", pos);
            return 2;
        }
        for (int i = 0; i < 4; ++i) {
            w[i] = 0;
            for (int b = 0; b < 8; ++b)
                w[i] |= (uint64_t)data[pos + 8 * (size_t)i + (size_t)b] << (8 * b);
        }
        pos += sizeof w;
        if (w[2] == 0 || (w[1] != 0 && w[0] > (data.size() - pos) / w[1])) {
            fprintf(stderr, "blob at byte %zu: piece limit 0, or frames past the end of the file\n", pos - sizeof w);
            return 2;
        }
        puts(scan_call(data.data() + pos, (size_t)w[0], (size_t)w[1], (size_t)w[2], w[3] != 0, argc > 2).c_str());
        pos += (size_t)(w[0] * w[1]);
    }
    return 0;
}
