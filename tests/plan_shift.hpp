// plan_shift.hpp — the shift case of the stand-alone plan checks
// (tests/*_plan_check.cpp): a plan takes addresses as plain integers and never
// dereferences them, so the same call can be planned with offsets X, with
// every offset X + D, and with the bases moved by D and offsets X, for D past
// 2^32.  Every 64-bit word of the tables must then be the first plan's or the
// first plan's plus D (an address or offset field), nothing else: a field
// narrowed to 32 bits on its way into a table differs by D mod 2^32 or by
// nothing where it should differ by D.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

namespace plan_shift {

// multiples of 256, so every alignment rule gives the same verdict
static const uint64_t SHIFTS[3] = {1ull << 32, (1ull << 32) + 768, 1ull << 40};

template <class T>
inline std::vector<T> moved(const std::vector<T> &x, uint64_t d) {
    std::vector<T> y(x);
    for (T &v : y) v = (T)(v + d);
    return y;
}

// The words of b that are a's plus d, counted; -1 where a word is neither
// a's nor a's plus d, or the sizes differ.  Tables are read in 8-byte words
// from their first byte (the structs in them are 8-byte aligned).
inline long shifted_words(const void *a, const void *b, size_t bytes, uint64_t d) {
    long n = 0;
    for (size_t i = 0; i + 8 <= bytes; i += 8) {
        uint64_t x, y;
        std::memcpy(&x, (const uint8_t *)a + i, 8);
        std::memcpy(&y, (const uint8_t *)b + i, 8);
        if (y == x) continue;
        if (y != x + d) return -1;
        ++n;
    }
    if (bytes % 8 && std::memcmp((const uint8_t *)a + bytes / 8 * 8, (const uint8_t *)b + bytes / 8 * 8, bytes % 8)) return -1;
    return n;
}

inline long shifted_words(const std::vector<uint8_t> &a, const std::vector<uint8_t> &b, uint64_t d) {
    return a.size() == b.size() ? shifted_words(a.data(), b.data(), a.size(), d) : -1;
}

template <class T>
inline long shifted_records(const T *a, const T *b, size_t count, uint64_t d) {
    static_assert(sizeof(T) % 8 == 0, "records of whole 8-byte words");
    return shifted_words((const void *)a, (const void *)b, count * sizeof(T), d);
}

}  // namespace plan_shift
