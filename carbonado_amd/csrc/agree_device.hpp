// agree_device.hpp — the key agreement of the Ecies stage as the kernels of
// agree_kernels.hip (KY) run it: secp256k1 scalar multiplication and
// HKDF-SHA256, written so that no load or store address and no branch depends
// on a secret.  Secret are: the ephemeral scalars, the receiver's secret
// scalar, every window digit, every intermediate and shared point, the HKDF
// state and the derived key.  Public are: the ephemeral PUBLIC keys, the
// receiver's public key and every table of multiples of a public point, lane
// and object indices, lengths, status words.  Parsing a 65-byte key branches
// freely: it only sees public bytes.
//
// Every function is __host__ __device__: the kernels and the stand-alone
// check tests/agree_device_check.cpp compile this same text, the check
// walking a multiplication lane by lane exactly as the kernels split it.
//
// Field.  An element is eight 32-bit limbs, little-endian, holding ANY value
// below 2^256 ("weakly reduced": p <= value is allowed, the representative is
// not unique).  Every operation accepts and returns such values, so there are
// no magnitudes to track: the largest input a point formula can feed in is
// 2^256 - 1.  Reduction uses 2^256 = 2^32 + 977 (mod p):
//   fe_mul   the 16-limb product t = lo + 2^256 hi < 2^512 folds to
//            lo + hi (2^32 + 977) < 2^256 + 2^289.1: eight limbs and a top
//            T < 2^33; T (2^32 + 977) < 2^66 is added in, which carries out
//            at most once (c <= 1); after that carry the eight limbs hold
//            less than 2^66, so adding c (2^32 + 977) cannot carry again.
//   fe_add   a + b < 2^257: carry c, then c (2^32 + 977) added twice over
//            (the first addition can carry when a + b >= 2^257 - 2^32 - 977;
//            the wrapped value is then below 2^33 and the second cannot).
//   fe_sub   a - b > -2^256: borrow c, then c (2^32 + 977) subtracted twice
//            over (the first can borrow when a - b + 2^256 < 2^32 + 977; the
//            wrapped value is then above 2^256 - 2^33 and the second cannot).
//   fe_small a k for k <= 2^16: eight limbs and a top T < 2^16, folded as in
//            fe_mul.
//   fe_norm  the unique representative in [0, p): value < 2^256 < 2 p, so p
//            is subtracted once under a mask (value + 2^32 + 977 carries out
//            iff value >= p).
// fe_inv is the fixed addition chain of k1::fe_inv (255 squarings, 15
// multiplications), run as one loop of 15 steps so that the kernels hold one
// copy of the multiplication.
//
// Points.  Projective (X : Y : Z), infinity (0 : 1 : 0), the complete
// formulas of Renes, Costello and Batina (EUROCRYPT 2016), Algorithms 7 and 9
// for a = 0, b3 = 21, as k1::pt_add / k1::pt_dbl: infinity, P + P and
// P + (-P) take the same path as everything else.
//
// Scalar multiplication, two shapes.
//   fixed base (comb_pick): the table holds i 16^j B for j < 64, i < 16 as 24
//            words each (X, Y, Z limbs), entry (j, i) at word 24 (16 j + i).
//            Lane j of a wave reads ALL 16 entries of row j and keeps entry
//            w_j under masks; the 64 picks are added in a 6-level butterfly
//            (lane l adds the point of lane l ^ m, m = 1, 2, .. 32), after
//            which every lane holds k B.
//   variable base (var_table / var_mul): one lane per point R.  The lane's 16
//            multiples of R (public) live in the call's scratch, word k of
//            entry i of object o at var_index(o, i, k), interleaved by lane
//            so that a wave's loads coalesce.  64 steps from the top window
//            down: four doublings, a masked scan of all 16 entries, one
//            addition.  Every step runs whatever the scalar.
//
// HKDF-SHA256 without salt or info, 32 bytes out, over the 130 bytes
// eph65 || shared65 (hkdf_points: the bytes are assembled in registers from
// the coordinates' limbs), and for the check over any byte string (hkdf32).
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KY_HD __host__ __device__ inline
#define KY_UNROLL _Pragma("unroll")
#define KY_ROLLED _Pragma("unroll 1")
#else
#define KY_HD inline
#define KY_UNROLL
#define KY_ROLLED
#endif

namespace chip {
namespace agree {

constexpr uint32_t LANES = 64;
constexpr uint32_t PT_WORDS = 24;                       // X, Y, Z limbs of a table entry
constexpr uint32_t COMB_WORDS = 64 * 16 * PT_WORDS;     // a fixed-base table (96 KiB)
constexpr uint32_t VAR_WORDS = 16 * PT_WORDS;           // a lane's table of multiples of R
constexpr uint32_t ERR_ECIES = 17;                      // CHIP_ERR_ECIES

struct Fe {
    uint32_t v[8];
};

constexpr uint32_t FOLD = 977;  // 2^256 = 2^32 + FOLD (mod p)

KY_HD Fe fe_zero() { return Fe{{0, 0, 0, 0, 0, 0, 0, 0}}; }
KY_HD Fe fe_one() { return Fe{{1, 0, 0, 0, 0, 0, 0, 0}}; }
KY_HD Fe fe_set(uint32_t x) { return Fe{{x, 0, 0, 0, 0, 0, 0, 0}}; }

// r += c (2^32 + 977) for c <= 1; the carry out
KY_HD uint32_t fe_fold_carry(Fe &r, uint32_t c) {
    uint64_t acc = uint64_t(r.v[0]) + uint64_t(c) * FOLD;
    r.v[0] = uint32_t(acc);
    acc = (acc >> 32) + r.v[1] + c;
    r.v[1] = uint32_t(acc);
    KY_UNROLL
    for (int i = 2; i < 8; ++i) {
        acc = (acc >> 32) + r.v[i];
        r.v[i] = uint32_t(acc);
    }
    return uint32_t(acc >> 32);
}

// r -= c (2^32 + 977) for c <= 1; the borrow out
KY_HD uint32_t fe_fold_borrow(Fe &r, uint32_t c) {
    uint64_t acc = uint64_t(r.v[0]) - uint64_t(c) * FOLD;
    r.v[0] = uint32_t(acc);
    acc = uint64_t(r.v[1]) - c - ((acc >> 32) & 1u);
    r.v[1] = uint32_t(acc);
    KY_UNROLL
    for (int i = 2; i < 8; ++i) {
        acc = uint64_t(r.v[i]) - ((acc >> 32) & 1u);
        r.v[i] = uint32_t(acc);
    }
    return uint32_t(acc >> 32) & 1u;
}

// eight limbs r and a top T < 2^34 above them -> r + T (2^32 + 977), weakly reduced
KY_HD Fe fe_fold_top(Fe r, uint64_t T) {
    const uint32_t tl = uint32_t(T), th = uint32_t(T >> 32);
    uint64_t acc = uint64_t(r.v[0]) + T * FOLD;  // < 2^32 + 2^44
    r.v[0] = uint32_t(acc);
    acc = (acc >> 32) + r.v[1] + tl;
    r.v[1] = uint32_t(acc);
    acc = (acc >> 32) + r.v[2] + th;
    r.v[2] = uint32_t(acc);
    KY_UNROLL
    for (int i = 3; i < 8; ++i) {
        acc = (acc >> 32) + r.v[i];
        r.v[i] = uint32_t(acc);
    }
    (void)fe_fold_carry(r, uint32_t(acc >> 32));
    return r;
}

KY_HD Fe fe_mul(const Fe &a, const Fe &b) {
    uint32_t t[16];
    KY_UNROLL
    for (int i = 0; i < 16; ++i) t[i] = 0;
    KY_UNROLL
    for (int i = 0; i < 8; ++i) {
        uint32_t c = 0;
        KY_UNROLL
        for (int j = 0; j < 8; ++j) {  // (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1: no overflow
            const uint64_t acc = uint64_t(a.v[i]) * b.v[j] + t[i + j] + c;
            t[i + j] = uint32_t(acc);
            c = uint32_t(acc >> 32);
        }
        t[i + 8] = c;
    }
    // lo + hi 977 + (hi << 32): the carry stays below 980
    Fe r;
    uint64_t acc = 0;
    KY_UNROLL
    for (int i = 0; i < 8; ++i) {
        acc += uint64_t(t[i]) + uint64_t(t[8 + i]) * FOLD + (i ? t[7 + i] : 0u);
        r.v[i] = uint32_t(acc);
        acc >>= 32;
    }
    return fe_fold_top(r, acc + t[15]);
}

KY_HD Fe fe_sqr(const Fe &a) { return fe_mul(a, a); }

KY_HD Fe fe_add(const Fe &a, const Fe &b) {
    Fe r;
    uint64_t acc = 0;
    KY_UNROLL
    for (int i = 0; i < 8; ++i) {
        acc += uint64_t(a.v[i]) + b.v[i];
        r.v[i] = uint32_t(acc);
        acc >>= 32;
    }
    const uint32_t c = fe_fold_carry(r, uint32_t(acc));
    (void)fe_fold_carry(r, c);
    return r;
}

KY_HD Fe fe_sub(const Fe &a, const Fe &b) {
    Fe r;
    uint64_t acc = 0;
    KY_UNROLL
    for (int i = 0; i < 8; ++i) {
        acc = uint64_t(a.v[i]) - b.v[i] - ((acc >> 32) & 1u);
        r.v[i] = uint32_t(acc);
    }
    const uint32_t c = fe_fold_borrow(r, uint32_t(acc >> 32) & 1u);
    (void)fe_fold_borrow(r, c);
    return r;
}

// a k for a small constant k <= 2^16
KY_HD Fe fe_small(const Fe &a, uint32_t k) {
    Fe r;
    uint64_t acc = 0;
    KY_UNROLL
    for (int i = 0; i < 8; ++i) {
        acc += uint64_t(a.v[i]) * k;
        r.v[i] = uint32_t(acc);
        acc >>= 32;
    }
    return fe_fold_top(r, acc);
}

KY_HD Fe fe_norm(const Fe &a) {
    Fe u;
    uint64_t acc = uint64_t(a.v[0]) + FOLD;
    u.v[0] = uint32_t(acc);
    acc = (acc >> 32) + a.v[1] + 1u;
    u.v[1] = uint32_t(acc);
    KY_UNROLL
    for (int i = 2; i < 8; ++i) {
        acc = (acc >> 32) + a.v[i];
        u.v[i] = uint32_t(acc);
    }
    const uint32_t ge = 0u - uint32_t(acc >> 32);  // all ones: a >= p, keep a + 2^256 - p mod 2^256
    Fe r;
    KY_UNROLL
    for (int i = 0; i < 8; ++i) r.v[i] = (u.v[i] & ge) | (a.v[i] & ~ge);
    return r;
}

// m all ones: b, m zero: a
KY_HD Fe fe_cmov(const Fe &a, const Fe &b, uint32_t m) {
    Fe r;
    KY_UNROLL
    for (int i = 0; i < 8; ++i) r.v[i] = (a.v[i] & ~m) | (b.v[i] & m);
    return r;
}

// all ones iff a = 0 (mod p)
KY_HD uint32_t fe_zero_mask(const Fe &a) {
    const Fe n = fe_norm(a);
    uint32_t o = 0;
    KY_UNROLL
    for (int i = 0; i < 8; ++i) o |= n.v[i];
    return uint32_t((uint64_t(o) - 1) >> 32);
}

KY_HD Fe fe_from_be(const uint8_t b[32]) {
    Fe r;
    KY_UNROLL
    for (int i = 0; i < 8; ++i) {
        const uint8_t *q = b + 4 * (7 - i);
        r.v[i] = (uint32_t(q[0]) << 24) | (uint32_t(q[1]) << 16) | (uint32_t(q[2]) << 8) | q[3];
    }
    return r;
}

KY_HD void fe_to_be(const Fe &a, uint8_t b[32]) {
    const Fe n = fe_norm(a);
    KY_UNROLL
    for (int i = 0; i < 8; ++i) {
        uint8_t *q = b + 4 * (7 - i);
        q[0] = uint8_t(n.v[i] >> 24), q[1] = uint8_t(n.v[i] >> 16), q[2] = uint8_t(n.v[i] >> 8), q[3] = uint8_t(n.v[i]);
    }
}

// step i of the chain of k1::fe_inv: n squarings, then times a saved power
// (0: a, 1: x2, 2: x3, 3: x22, 4: x44, 5: the value the step began with), the
// result saved as (1: x2, 2: x3, 3: x22, 4: x44, 0: not saved)
KY_HD void fe_inv_step(int i, uint32_t &n, uint32_t &mul, uint32_t &save) {
    switch (i) {
    case 0: n = 1, mul = 0, save = 1; break;    // x2
    case 1: n = 1, mul = 0, save = 2; break;    // x3
    case 2: n = 3, mul = 2, save = 0; break;    // x6
    case 3: n = 3, mul = 2, save = 0; break;    // x9
    case 4: n = 2, mul = 1, save = 0; break;    // x11
    case 5: n = 11, mul = 5, save = 3; break;   // x22
    case 6: n = 22, mul = 5, save = 4; break;   // x44
    case 7: n = 44, mul = 5, save = 0; break;   // x88
    case 8: n = 88, mul = 5, save = 0; break;   // x176
    case 9: n = 44, mul = 4, save = 0; break;   // x220
    case 10: n = 3, mul = 2, save = 0; break;   // x223
    case 11: n = 23, mul = 3, save = 0; break;
    case 12: n = 5, mul = 0, save = 0; break;
    case 13: n = 3, mul = 1, save = 0; break;
    default: n = 2, mul = 0, save = 0; break;
    }
}

// a^(p - 2); 0 for a = 0.  The step table is public, the selections by masks.
KY_HD Fe fe_inv(const Fe &a) {
    Fe t = a, x2 = a, x3 = a, x22 = a, x44 = a;
    KY_ROLLED
    for (int i = 0; i < 15; ++i) {
        uint32_t n, mul, save;
        fe_inv_step(i, n, mul, save);
        Fe m = t;  // mul == 5
        m = fe_cmov(m, a, 0u - uint32_t(mul == 0));
        m = fe_cmov(m, x2, 0u - uint32_t(mul == 1));
        m = fe_cmov(m, x3, 0u - uint32_t(mul == 2));
        m = fe_cmov(m, x22, 0u - uint32_t(mul == 3));
        m = fe_cmov(m, x44, 0u - uint32_t(mul == 4));
        // n squarings and the multiplication share one fe_mul: the last round multiplies by m
        KY_ROLLED
        for (uint32_t s = 0; s <= n; ++s) t = fe_mul(t, fe_cmov(t, m, 0u - uint32_t(s == n)));
        x2 = fe_cmov(x2, t, 0u - uint32_t(save == 1));
        x3 = fe_cmov(x3, t, 0u - uint32_t(save == 2));
        x22 = fe_cmov(x22, t, 0u - uint32_t(save == 3));
        x44 = fe_cmov(x44, t, 0u - uint32_t(save == 4));
    }
    return t;
}

// ---- points ---------------------------------------------------------------------
struct Pt {
    Fe x, y, z;
};

KY_HD Pt pt_inf() { return Pt{fe_zero(), fe_one(), fe_zero()}; }

KY_HD Fe fe_mul21(const Fe &a) { return fe_small(a, 21); }

// Renes-Costello-Batina Algorithm 7 (a = 0): complete addition
KY_HD Pt pt_add(const Pt &p, const Pt &q) {
    Fe t0 = fe_mul(p.x, q.x), t1 = fe_mul(p.y, q.y), t2 = fe_mul(p.z, q.z);
    Fe t3 = fe_add(p.x, p.y), t4 = fe_add(q.x, q.y);
    t3 = fe_mul(t3, t4);
    t4 = fe_add(t0, t1);
    t3 = fe_sub(t3, t4);
    t4 = fe_add(p.y, p.z);
    Fe x3 = fe_add(q.y, q.z);
    t4 = fe_mul(t4, x3);
    x3 = fe_add(t1, t2);
    t4 = fe_sub(t4, x3);
    x3 = fe_add(p.x, p.z);
    Fe y3 = fe_add(q.x, q.z);
    x3 = fe_mul(x3, y3);
    y3 = fe_add(t0, t2);
    y3 = fe_sub(x3, y3);
    x3 = fe_add(t0, t0);
    t0 = fe_add(x3, t0);
    t2 = fe_mul21(t2);
    Fe z3 = fe_add(t1, t2);
    t1 = fe_sub(t1, t2);
    y3 = fe_mul21(y3);
    x3 = fe_mul(t4, y3);
    t2 = fe_mul(t3, t1);
    x3 = fe_sub(t2, x3);
    y3 = fe_mul(y3, t0);
    t1 = fe_mul(t1, z3);
    y3 = fe_add(t1, y3);
    t0 = fe_mul(t0, t3);
    z3 = fe_mul(z3, t4);
    z3 = fe_add(z3, t0);
    return Pt{x3, y3, z3};
}

// Renes-Costello-Batina Algorithm 9 (a = 0): complete doubling
KY_HD Pt pt_dbl(const Pt &p) {
    Fe t0 = fe_sqr(p.y);
    Fe z3 = fe_small(t0, 8);
    Fe t1 = fe_mul(p.y, p.z), t2 = fe_sqr(p.z);
    t2 = fe_mul21(t2);
    Fe x3 = fe_mul(t2, z3), y3 = fe_add(t0, t2);
    z3 = fe_mul(t1, z3);
    t1 = fe_add(t2, t2);
    t2 = fe_add(t1, t2);
    t0 = fe_sub(t0, t2);
    y3 = fe_mul(t0, y3);
    y3 = fe_add(x3, y3);
    t1 = fe_mul(p.x, p.y);
    x3 = fe_mul(t0, t1);
    x3 = fe_add(x3, x3);
    return Pt{x3, y3, z3};
}

// all ones iff i == w (i, w < 2^31)
KY_HD uint32_t eq_mask(uint32_t i, uint32_t w) { return 0u - (((i ^ w) - 1u) >> 31); }

// j-th 4-bit window of a scalar held as eight little-endian words, from the one
// word that holds it: the caller loads kw = words[j >> 3] (a public address)
KY_HD uint32_t window_of(uint32_t kw, uint32_t j) { return (kw >> (4 * (j & 7u))) & 15u; }

// Row j of a fixed-base table: every one of its 16 entries read, entry w kept.
KY_HD Pt comb_pick(const uint32_t *table, uint32_t j, uint32_t w) {
    const uint32_t *row = table + size_t(j) * 16 * PT_WORDS;
    Pt r{fe_zero(), fe_zero(), fe_zero()};
    KY_ROLLED
    for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t m = eq_mask(i, w);
        const uint32_t *e = row + i * PT_WORDS;
        KY_UNROLL
        for (int k = 0; k < 8; ++k) {
            r.x.v[k] |= e[k] & m;
            r.y.v[k] |= e[8 + k] & m;
            r.z.v[k] |= e[16 + k] & m;
        }
    }
    return r;
}

// word k of entry i of object o's table of multiples (var_table / var_mul)
KY_HD size_t var_index(uint64_t o, uint32_t i, uint32_t k) {
    return (size_t(o / LANES) * VAR_WORDS + i * PT_WORDS + k) * LANES + size_t(o % LANES);
}

// the scratch words a call's tables of multiples take
KY_HD uint64_t var_words(uint64_t count) { return (count + LANES - 1) / LANES * LANES * VAR_WORDS; }

KY_HD void var_store(uint32_t *tab, uint64_t o, uint32_t i, const Pt &p) {
    KY_UNROLL
    for (int k = 0; k < 8; ++k) {
        tab[var_index(o, i, k)] = p.x.v[k];
        tab[var_index(o, i, 8 + k)] = p.y.v[k];
        tab[var_index(o, i, 16 + k)] = p.z.v[k];
    }
}

// i R for i < 16 of the affine point R = (x, y) (public) into object o's table
KY_HD void var_table(uint32_t *tab, uint64_t o, const Fe &x, const Fe &y) {
    const Pt base{x, y, fe_one()};
    Pt acc = pt_inf();
    KY_ROLLED
    for (uint32_t i = 0; i < 16; ++i) {
        var_store(tab, o, i, acc);
        acc = pt_add(acc, base);
    }
}

KY_HD Pt var_pick(const uint32_t *tab, uint64_t o, uint32_t w) {
    Pt r{fe_zero(), fe_zero(), fe_zero()};
    KY_ROLLED
    for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t m = eq_mask(i, w);
        KY_UNROLL
        for (int k = 0; k < 8; ++k) {
            r.x.v[k] |= tab[var_index(o, i, k)] & m;
            r.y.v[k] |= tab[var_index(o, i, 8 + k)] & m;
            r.z.v[k] |= tab[var_index(o, i, 16 + k)] & m;
        }
    }
    return r;
}

// k R from object o's table; k as eight little-endian words at a public address
KY_HD Pt var_mul(const uint32_t *tab, uint64_t o, const uint32_t *k) {
    Pt r = pt_inf();
    KY_ROLLED
    for (int j = 63; j >= 0; --j) {
        KY_ROLLED
        for (int d = 0; d < 4; ++d) r = pt_dbl(r);
        r = pt_add(r, var_pick(tab, o, window_of(k[j >> 3], uint32_t(j))));
    }
    return r;
}

// the affine coordinates of two points with one inversion (zeros for infinity)
KY_HD void affine_pair(const Pt &p, const Pt &q, Fe &px, Fe &py, Fe &qx, Fe &qy) {
    const Fe i = fe_inv(fe_mul(p.z, q.z));
    const Fe pi = fe_mul(i, q.z), qi = fe_mul(i, p.z);
    px = fe_norm(fe_mul(p.x, pi));
    py = fe_norm(fe_mul(p.y, pi));
    qx = fe_norm(fe_mul(q.x, qi));
    qy = fe_norm(fe_mul(q.y, qi));
}

KY_HD void affine(const Pt &p, Fe &x, Fe &y) {
    const Fe i = fe_inv(p.z);
    x = fe_norm(fe_mul(p.x, i));
    y = fe_norm(fe_mul(p.y, i));
}

// ---- parsing a 65-byte key (public bytes: branches are fine) ------------------------
// 0x04 as k1::parse_full: both coordinates below p and y^2 = x^3 + 7.  0x06 / 0x07
// (the hybrid form) as OpenSSL's EC_POINT_oct2point: the same, and the low bit
// of y equal to the low bit of the prefix.  Everything else is refused.
KY_HD bool fe_below_p(const Fe &a) {
    const Fe n = fe_norm(a);
    bool same = true;
    for (int i = 0; i < 8; ++i) same = same && n.v[i] == a.v[i];
    return same;
}

KY_HD uint32_t parse65(const uint8_t in[65], Fe &x, Fe &y) {
    const uint8_t tag = in[0];
    if (tag != 0x04 && tag != 0x06 && tag != 0x07) return ERR_ECIES;
    x = fe_from_be(in + 1);
    y = fe_from_be(in + 33);
    if (!fe_below_p(x) || !fe_below_p(y)) return ERR_ECIES;
    const Fe rhs = fe_add(fe_mul(fe_sqr(x), x), fe_set(7));
    if (!fe_zero_mask(fe_sub(fe_sqr(y), rhs))) return ERR_ECIES;
    if (tag != 0x04 && (y.v[0] & 1u) != (tag & 1u)) return ERR_ECIES;
    return 0;
}

// ---- SHA-256, HMAC, HKDF ------------------------------------------------------------
KY_HD uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

KY_HD uint32_t sha_k(uint32_t i) {
    static constexpr uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
        0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
        0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
        0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
        0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
        0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
        0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
        0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    return K[i];
}

struct Sha {
    uint32_t h[8];
};
struct Block {
    uint32_t w[16];  // big-endian words of 64 message bytes
};

KY_HD Sha sha_init() {
    return Sha{{0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19}};
}

// One block.  Four passes of 16 rounds: the schedule lives in w[16] at static
// indices, the round constant's address depends on the pass alone.
KY_HD void sha_compress(Sha &s, Block b) {
    uint32_t a = s.h[0], bb = s.h[1], c = s.h[2], d = s.h[3], e = s.h[4], f = s.h[5], g = s.h[6], h = s.h[7];
    KY_ROLLED
    for (uint32_t t = 0; t < 4; ++t) {
        KY_UNROLL
        for (int i = 0; i < 16; ++i) {
            if (t) {
                const uint32_t w15 = b.w[(i + 1) & 15], w2 = b.w[(i + 14) & 15];
                b.w[i] += (rotr(w15, 7) ^ rotr(w15, 18) ^ (w15 >> 3)) + b.w[(i + 9) & 15] +
                          (rotr(w2, 17) ^ rotr(w2, 19) ^ (w2 >> 10));
            }
            const uint32_t t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) +
                                sha_k(16 * t + i) + b.w[i];
            const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & bb) ^ (a & c) ^ (bb & c));
            h = g, g = f, f = e, e = d + t1, d = c, c = bb, bb = a, a = t1 + t2;
        }
    }
    s.h[0] += a, s.h[1] += bb, s.h[2] += c, s.h[3] += d, s.h[4] += e, s.h[5] += f, s.h[6] += g, s.h[7] += h;
}

// the key block of an HMAC whose key is eight words (zero words: no salt) under the pad byte
KY_HD Block hmac_pad(const uint32_t key[8], uint32_t pad) {
    Block b;
    KY_UNROLL
    for (int i = 0; i < 16; ++i) b.w[i] = (i < 8 ? key[i] : 0u) ^ pad;
    return b;
}

// SHA-256(opad block || inner digest)
KY_HD Sha hmac_outer(const uint32_t key[8], const Sha &inner) {
    Sha s = sha_init();
    sha_compress(s, hmac_pad(key, 0x5c5c5c5cu));
    Block b;
    KY_UNROLL
    for (int i = 0; i < 8; ++i) b.w[i] = inner.h[i];
    b.w[8] = 0x80000000u;
    KY_UNROLL
    for (int i = 9; i < 15; ++i) b.w[i] = 0;
    b.w[15] = (64 + 32) * 8;
    sha_compress(s, b);
    return s;
}

// T(1) of HKDF-Expand without info from the pseudorandom key: HMAC(prk, 0x01)
KY_HD Sha hkdf_expand32(const Sha &prk) {
    Sha s = sha_init();
    sha_compress(s, hmac_pad(prk.h, 0x36363636u));
    Block b;
    b.w[0] = 0x01800000u;
    KY_UNROLL
    for (int i = 1; i < 15; ++i) b.w[i] = 0;
    b.w[15] = (64 + 1) * 8;
    sha_compress(s, b);
    return hmac_outer(prk.h, s);
}

// HKDF(tag || ex || ey || 0x04 || sx || sy) -> 32 bytes as eight big-endian
// words.  The coordinates are normalised field elements; word 7 - i of a
// coordinate's big-endian bytes is its limb i.
KY_HD Sha hkdf_points(uint32_t tag, const Fe &ex, const Fe &ey, const Fe &sx, const Fe &sy) {
    uint32_t A[16], B[16];
    KY_UNROLL
    for (int i = 0; i < 8; ++i) {
        A[i] = ex.v[7 - i], A[8 + i] = ey.v[7 - i];
        B[i] = sx.v[7 - i], B[8 + i] = sy.v[7 - i];
    }
    const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    Sha s = sha_init();
    sha_compress(s, hmac_pad(zero, 0x36363636u));
    Block b;
    b.w[0] = (tag << 24) | (A[0] >> 8);  // byte 0 the tag, bytes 1 .. 64 the ephemeral coordinates
    KY_UNROLL
    for (int i = 1; i < 16; ++i) b.w[i] = (A[i - 1] << 24) | (A[i] >> 8);
    sha_compress(s, b);
    b.w[0] = (A[15] << 24) | (0x04u << 16) | (B[0] >> 16);  // byte 65 the 0x04, bytes 66 .. 129 the shared point
    KY_UNROLL
    for (int i = 1; i < 16; ++i) b.w[i] = (B[i - 1] << 16) | (B[i] >> 16);
    sha_compress(s, b);
    b.w[0] = (B[15] << 16) | 0x8000u;
    KY_UNROLL
    for (int i = 1; i < 15; ++i) b.w[i] = 0;
    b.w[15] = (64 + 130) * 8;
    sha_compress(s, b);
    return hkdf_expand32(hmac_outer(zero, s));
}

KY_HD void sha_to_be(const Sha &s, uint8_t out[32]) {
    KY_UNROLL
    for (int i = 0; i < 8; ++i) {
        out[4 * i] = uint8_t(s.h[i] >> 24), out[4 * i + 1] = uint8_t(s.h[i] >> 16);
        out[4 * i + 2] = uint8_t(s.h[i] >> 8), out[4 * i + 3] = uint8_t(s.h[i]);
    }
}

// The same HKDF over any byte string (the stand-alone check: RFC 5869 and the
// comparison with hkdf_points); its loads follow the length, which is public.
KY_HD void hkdf32(const uint8_t *ikm, size_t len, uint8_t out[32]) {
    const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    Sha s = sha_init();
    sha_compress(s, hmac_pad(zero, 0x36363636u));
    const size_t padded = (len + 9 + 63) / 64 * 64;
    const uint64_t bits = uint64_t(64 + len) * 8;
    for (size_t at = 0; at < padded; at += 64) {
        Block b;
        for (int i = 0; i < 16; ++i) {
            uint32_t w = 0;
            for (int k = 0; k < 4; ++k) {
                const size_t p = at + 4 * size_t(i) + size_t(k);
                uint32_t byte = p < len ? ikm[p] : (p == len ? 0x80u : 0u);
                if (p >= padded - 8) byte = uint32_t(bits >> (8 * (padded - 1 - p))) & 0xFFu;
                w = (w << 8) | byte;
            }
            b.w[i] = w;
        }
        sha_compress(s, b);
    }
    sha_to_be(hkdf_expand32(hmac_outer(zero, s)), out);
}

}  // namespace agree
}  // namespace chip
