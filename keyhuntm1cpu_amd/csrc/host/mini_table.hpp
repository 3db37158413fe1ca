// The window table of the device's fixed-base multiplication (device/minikey.hpp mini_mul_g, khb_load_mini_table).
#pragma once
#include <stdint.h>

#include <vector>

namespace khb {

// d * 2^(w j) * G for j = 0 .. 256/w - 1 and d = 1 .. 2^w - 1 in that order, x||y big-endian, 64 bytes each; w = 4, 8
// or 16 (empty otherwise).  Each window's points are built by doubling the filled part, point m + i = point i +
// point m for i <= m, with one batch inversion per step; the windows are shared among `threads` threads.
std::vector<uint8_t> mini_table_be(uint32_t window_bits, int threads);

}  // namespace khb
