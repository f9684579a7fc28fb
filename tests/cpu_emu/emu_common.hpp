// emu_common.hpp -- what every part of the CPU emulation of the tile functions shares: the emulation switch, the filter-bank
// setters, the list of even filter lengths.  Test infrastructure; never shipped.
#pragma once
#define PDWT_CPU_EMU 1
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../pypwt_amd/csrc/packed_math.hpp"

using namespace pdwt;

#define EMU_API extern "C" __attribute__((visibility("default")))

// Elements of slack some runners add behind the emulated LDS and the scratch planes.  The sanitizer programs (emu_san.cpp) build
// with 0: there the LDS is the geometry's size to the element, and a read behind it is a finding.
#ifndef EMU_SLACK
#define EMU_SLACK 64
#endif

[[maybe_unused]] static void set_bank(FilterBank& fb, const float* lo, const float* hi, int hlen) {
    std::memset(&fb, 0, sizeof(fb));
    for (int i = 0; i < hlen; i++) { fb.lo[i] = lo[i]; fb.hi[i] = hi[i]; }
}

[[maybe_unused]] static void set_bank_i(FilterBankI& fb, const float* lo, const float* hi, int hlen) {
    std::memset(&fb, 0, sizeof(fb));
    for (int i = 0; i < hlen; i++) { fb.t[i].x = lo[i]; fb.t[i].y = hi[i]; }
}

[[maybe_unused]] static void interleave_bank(FilterBankI& o, const float* lo, const float* hi, int hlen) {
    std::memset(&o, 0, sizeof(o));
    for (int i = 0; i < hlen; i++) { o.t[i].x = lo[i]; o.t[i].y = hi[i]; }
}

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

#define EMU_EVEN_HLENS(X) X(2) X(4) X(6) X(8) X(10) X(12) X(14) X(16) X(18) X(20) X(22) X(24) X(26) \
    X(28) X(30) X(32) X(34) X(36) X(38) X(40)
