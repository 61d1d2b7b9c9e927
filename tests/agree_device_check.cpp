// agree_device_check.cpp — the text the KY kernels compile
// (carbonado_amd/csrc/agree_device.hpp) and the host's share
// (agree_plan.hpp), run on the host as a stand-alone program under
// ASan + UBSan (tests/test_agree_cpu.py).  It answers the requests of a vector
// file, one per line, and the test compares the answers with Python integers,
// the Python oracle's secp256k1 and hashlib:
//   fe OP A B        one field operation on 32-byte big-endian values, given as
//                    they are (not reduced); the answer is the normalised result
//   seal K PX PY     the seal kernel's work for scalar K and receiver (PX, PY):
//                    64 lanes pick from the comb tables of G and P, the 6-level
//                    butterfly, one inversion, HKDF; answers pub65 and the key
//   open K EPH65     the open kernel's lane: parse, the table of multiples in an
//                    interleaved scratch of 130 objects, the fixed-window
//                    ladder, HKDF; answers the status and the key
//   hkdf BYTES       hkdf32 over any byte string; for 130 bytes also hkdf_points
//   scalar K         agree::scalar_ok
// and checks by itself that the 64 lanes of a butterfly end on the same point
// and that the var table of a neighbouring object is left alone.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "agree_plan.hpp"

using namespace chip;
using namespace chip::agree;

static int failures = 0;

static std::vector<uint8_t> unhex(const std::string &s) {
    std::vector<uint8_t> out;
    if (s == "-") return out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back(uint8_t(std::stoul(s.substr(i, 2), nullptr, 16)));
    return out;
}

static std::string hex(const uint8_t *p, size_t n) {
    static const char *d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) s += d[p[i] >> 4], s += d[p[i] & 15];
    return s;
}

static Fe fe_of(const std::string &s) {
    const std::vector<uint8_t> b = unhex(s);
    if (b.size() != 32) std::abort();
    return fe_from_be(b.data());
}

static std::string fe_hex(const Fe &f) {
    uint8_t b[32];
    fe_to_be(f, b);
    return hex(b, 32);
}

static bool same_point(const Pt &a, const Pt &b) {  // x1 z2 = x2 z1, y1 z2 = y2 z1
    return fe_zero_mask(fe_sub(fe_mul(a.x, b.z), fe_mul(b.x, a.z))) &&
           fe_zero_mask(fe_sub(fe_mul(a.y, b.z), fe_mul(b.y, a.z)));
}

// k B over the 64 lanes of a wave, as agree_seal_kernel does it
static Pt comb_wave(const uint32_t *table, const uint32_t kw[8]) {
    Pt p[LANES], q[LANES];
    for (uint32_t lane = 0; lane < LANES; ++lane) p[lane] = comb_pick(table, lane, window_of(kw[lane >> 3], lane));
    for (uint32_t m = 1; m < LANES; m <<= 1) {
        for (uint32_t lane = 0; lane < LANES; ++lane) q[lane] = pt_add(p[lane], p[lane ^ m]);
        for (uint32_t lane = 0; lane < LANES; ++lane) p[lane] = q[lane];
    }
    for (uint32_t lane = 1; lane < LANES; ++lane)
        if (!same_point(p[0], p[lane])) ++failures, std::printf("# lanes differ at %u\n", lane);
    return p[0];
}

static void scalar_of(const std::string &s, uint32_t kw[8]) {
    const std::vector<uint8_t> b = unhex(s);
    if (b.size() != 32) std::abort();
    uint8_t w[32];
    scalar_words(b.data(), w);
    std::memcpy(kw, w, 32);
}

static std::vector<uint32_t> comb_of(const k1::Fe &x, const k1::Fe &y) {
    auto t = std::make_unique<k1::CombTable>(x, y);
    std::vector<uint32_t> w(COMB_WORDS);
    fill_comb(*t, w.data());
    return w;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    const std::vector<uint32_t> gtab = comb_of(k1::gx(), k1::gy());
    std::vector<uint32_t> ptab;
    std::string ptab_key;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string cmd, a, b, c;
        ss >> cmd >> a >> b >> c;
        if (cmd == "fe") {
            const Fe x = fe_of(b), y = fe_of(c);
            Fe r = fe_zero();
            if (a == "mul") r = fe_mul(x, y);
            else if (a == "sqr") r = fe_sqr(x);
            else if (a == "add") r = fe_add(x, y);
            else if (a == "sub") r = fe_sub(x, y);
            else if (a == "mul21") r = fe_mul21(x);
            else if (a == "mul8") r = fe_small(x, 8);
            else if (a == "inv") r = fe_inv(x);
            else if (a == "norm") r = fe_norm(x);
            else if (a == "iszero") r = fe_set(fe_zero_mask(x) & 1u);
            else if (a == "cmov") r = fe_cmov(fe_cmov(x, y, 0xFFFFFFFFu), x, 0);  // y
            else std::abort();
            std::printf("%s\n", fe_hex(r).c_str());
        } else if (cmd == "seal") {
            uint32_t kw[8];
            scalar_of(a, kw);
            if (ptab_key != b + c) {
                uint8_t p65[65] = {4};
                std::memcpy(p65 + 1, unhex(b).data(), 32);
                std::memcpy(p65 + 33, unhex(c).data(), 32);
                k1::Fe x, y;
                if (!k1::parse_full(p65, x, y)) std::abort();
                ptab = comb_of(x, y);
                ptab_key = b + c;
            }
            const Pt e = comb_wave(gtab.data(), kw), s = comb_wave(ptab.data(), kw);
            Fe ex, ey, sx, sy;
            affine_pair(e, s, ex, ey, sx, sy);
            uint8_t key[32];
            sha_to_be(hkdf_points(4, ex, ey, sx, sy), key);
            std::printf("04%s%s %s%s %s\n", fe_hex(ex).c_str(), fe_hex(ey).c_str(), fe_hex(sx).c_str(),
                        fe_hex(sy).c_str(), hex(key, 32).c_str());
        } else if (cmd == "open") {
            uint32_t kw[8];
            scalar_of(a, kw);
            const std::vector<uint8_t> eph = unhex(b);
            if (eph.size() != 65) std::abort();
            const uint64_t count = 130, o = 70;  // the second wave's lane 6
            std::vector<uint32_t> vtab(var_words(count), 0xA5A5A5A5u);
            Fe x, y;
            const uint32_t st = parse65(eph.data(), x, y);
            uint8_t key[32] = {0};
            if (!st) {
                var_table(vtab.data(), o, x, y);
                for (uint32_t i = 0; i < 16; ++i)
                    for (uint32_t k = 0; k < PT_WORDS; ++k)
                        if (vtab[var_index(o + 1, i, k)] != 0xA5A5A5A5u || vtab[var_index(o - 64, i, k)] != 0xA5A5A5A5u)
                            ++failures;
                Fe sx, sy;
                affine(var_mul(vtab.data(), o, kw), sx, sy);
                sha_to_be(hkdf_points(eph[0], x, y, sx, sy), key);
            }
            std::printf("%u %s\n", st, hex(key, 32).c_str());
        } else if (cmd == "hkdf") {
            const std::vector<uint8_t> m = unhex(a);
            uint8_t key[32];
            hkdf32(m.data(), m.size(), key);
            std::string out = hex(key, 32);
            if (m.size() == 130) {
                uint8_t k2[32];
                sha_to_be(hkdf_points(m[0], fe_from_be(&m[1]), fe_from_be(&m[33]), fe_from_be(&m[66]), fe_from_be(&m[98])),
                          k2);
                out += " " + hex(k2, 32);
            }
            std::printf("%s\n", out.c_str());
        } else if (cmd == "scalar") {
            std::printf("%d\n", int(scalar_ok(unhex(a).data())));
        } else if (!cmd.empty()) {
            std::abort();
        }
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
