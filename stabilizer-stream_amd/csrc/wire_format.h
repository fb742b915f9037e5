// wire_format.h -- the payload layouts of stream frames by Format id (src/de/mod.rs:12-17), ONE table for the host runtime, the
// decode kernels and the CPU check programs.  Plain C++17, no HIP: constexpr functions are host and device under hipcc.
#pragma once

namespace psdk {

struct WireFmt {
    int id;
    int batch_bytes; // bytes per batch
    int spb;         // samples per batch and trace
    int ntraces;     // Payload::traces
    const char *name;
};

constexpr WireFmt WIRE_FMTS[4] = {
    {1, 64, 8, 4, "AdcDac"},        // [[[u8;2];8];4]  data.rs:13
    {2, 56, 1, 4, "Fls"},           // [[[u8;4];7];2]  data.rs:86
    {3, 80, 1, 4, "ThermostatEem"}, // [[u8;4];16+4]   data.rs:144
    {4, 24, 1, 3, "Mpll"},          // [[u8;4];6]      data.rs:168
};

constexpr bool wire_fmt_known(int id) { return id >= 1 && id <= 4; }

// the layout of a KNOWN id by value (usable as `constexpr WireFmt f = wire_fmt_v(FMT);` in a kernel template)
constexpr WireFmt wire_fmt_v(int id) { return WIRE_FMTS[id - 1]; }

// ... and of any id: nullptr for one that no format has (de::Error::UnknownFormat, src/de/frame.rs:30)
inline const WireFmt *wire_fmt(int id) { return wire_fmt_known(id) ? &WIRE_FMTS[id - 1] : nullptr; }

} // namespace psdk
