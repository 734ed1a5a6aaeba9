// ws_text.h -- the decimal text of the mesh writer, shared by the host and the gfx950 kernels (ws_mesh.hip).
//
// WriteMesh (reconstruction.cpp:72-149) writes a float with `out << float`, which libstdc++ turns into
// printf("%.6g", (double)f); counts and indices are plain unsigned decimals.  g_format() restates glibc's "%.6g" of a
// float exactly -- round-half-even on the float's exact binary value -- in integer arithmetic only: the value is
// m * 2^e (m < 2^24, e in [-149, 104]) and the six significant digits are the quotient of two big integers of at most
// 8 x 32 bits (Big), found by restoring division.  Header only; needs no HIP include under a host compiler, so the CPU
// test (tests/cxx/mesh_text_check.cpp) builds it with g++.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WS_TEXT_FN __host__ __device__ inline
#else
#define WS_TEXT_FN inline
#endif

namespace wsamd {
namespace text {

constexpr int kMaxG = 12; // longest g_format() text: "-1.23456e-45", "-0.000123456"

struct Big { // little-endian 32-bit words; every loop has a constant trip count so that the words stay in registers
    uint32_t w[8];
};

WS_TEXT_FN void big_set(Big &a, uint32_t v)
{
    a.w[0] = v;
    for (int i = 1; i < 8; ++i) a.w[i] = 0;
}

WS_TEXT_FN void big_shl(Big &a, int n) // n >= 0; the caller keeps the result below 2^256
{
    while (n >= 32) {
        for (int i = 7; i > 0; --i) a.w[i] = a.w[i - 1];
        a.w[0] = 0;
        n -= 32;
    }
    if (n == 0) return;
    for (int i = 7; i > 0; --i) a.w[i] = (a.w[i] << n) | (a.w[i - 1] >> (32 - n));
    a.w[0] <<= n;
}

WS_TEXT_FN void big_shr1(Big &a)
{
    for (int i = 0; i < 7; ++i) a.w[i] = (a.w[i] >> 1) | (a.w[i + 1] << 31);
    a.w[7] >>= 1;
}

WS_TEXT_FN void big_mul(Big &a, uint32_t v)
{
    uint64_t carry = 0;
    for (int i = 0; i < 8; ++i) {
        const uint64_t t = (uint64_t)a.w[i] * v + carry;
        a.w[i] = (uint32_t)t;
        carry = t >> 32;
    }
}

WS_TEXT_FN void big_mul_pow10(Big &a, int n) // n >= 0
{
    for (; n >= 9; n -= 9) big_mul(a, 1000000000u);
    uint32_t p = 1;
    for (; n > 0; --n) p *= 10;
    if (p != 1) big_mul(a, p);
}

WS_TEXT_FN int big_cmp(const Big &a, const Big &b)
{
    int r = 0;
    for (int i = 7; i >= 0; --i)
        if (r == 0 && a.w[i] != b.w[i]) r = a.w[i] < b.w[i] ? -1 : 1;
    return r;
}

WS_TEXT_FN void big_sub(Big &a, const Big &b) // a >= b
{
    uint32_t borrow = 0;
    for (int i = 0; i < 8; ++i) {
        const uint64_t t = (uint64_t)a.w[i] - b.w[i] - borrow;
        a.w[i] = (uint32_t)t;
        borrow = (uint32_t)(t >> 63);
    }
}

// floor(m * 2^e / 10^s) for a quotient below 2^22, and how the remainder compares with half the divisor (-1, 0, 1)
WS_TEXT_FN uint32_t scaled_quotient(uint32_t m, int e, int s, int *half)
{
    Big num, den;
    big_set(num, m);
    big_set(den, 1);
    if (e >= 0) big_shl(num, e); else big_shl(den, -e);
    if (s >= 0) big_mul_pow10(den, s); else big_mul_pow10(num, -s);
    big_shl(den, 21);
    uint32_t q = 0;
    for (int k = 21; k >= 0; --k) {
        if (big_cmp(num, den) >= 0) {
            big_sub(num, den);
            q |= 1u << k;
        }
        if (k > 0) big_shr1(den); // ends as the divisor itself
    }
    big_shl(num, 1); // 2 * remainder < 2 * divisor: fits
    *half = big_cmp(num, den);
    return q;
}

// A float as printf's %.6g sees it: kind 0 = finite non-zero (digits * 10^(exp10 - 5), digits in [1e5, 1e6)),
// 1 = zero, 2 = inf, 3 = nan; neg = the sign bit (glibc prints it for NaN and zero too)
struct G6 {
    int kind, neg, exp10;
    uint32_t digits;
};

WS_TEXT_FN G6 g6_decompose(float f)
{
    const uint32_t bits = __builtin_bit_cast(uint32_t, f);
    G6 r{0, (int)(bits >> 31), 0, 0};
    const uint32_t be = (bits >> 23) & 0xffu, frac = bits & 0x7fffffu;
    if (be == 0xffu) { r.kind = frac ? 3 : 2; return r; }
    if (be == 0 && frac == 0) { r.kind = 1; return r; }
    const uint32_t m = be ? (frac | 0x800000u) : frac;
    const int e = be ? (int)be - 150 : -149;
    const int p = 31 - __builtin_clz(m) + e;      // 2^p <= value < 2^(p+1)
    int x = (p * 78913) >> 18;                     // floor(p * log10(2)) for |p| < 1650: 10^x <= value
    int half;
    uint32_t q = scaled_quotient(m, e, x - 5, &half);
    if (q >= 1000000u) {                           // value >= 10^(x+1): x was one short
        ++x;
        q = scaled_quotient(m, e, x - 5, &half);
    }
    if (half > 0 || (half == 0 && (q & 1u))) ++q;  // round half to even on the exact value
    if (q == 1000000u) { q = 100000u; ++x; }       // the carry reaches the next power of ten
    r.digits = q;
    r.exp10 = x;
    return r;
}

WS_TEXT_FN int g6_sig_digits(uint32_t d) // significant digits left after %g drops trailing zeros
{
    int n = 6;
    while (n > 1 && d % 10u == 0) { d /= 10u; --n; }
    return n;
}

WS_TEXT_FN int g6_length(const G6 &g)
{
    if (g.kind == 1) return g.neg + 1;
    if (g.kind >= 2) return g.neg + 3;
    const int nd = g6_sig_digits(g.digits), x = g.exp10;
    if (x < -4 || x >= 6) {
        const int ax = x < 0 ? -x : x;
        return g.neg + 1 + (nd > 1 ? nd : 0) + 2 + (ax >= 100 ? 3 : 2);
    }
    if (x >= 0) return g.neg + (x + 1) + (nd > x + 1 ? nd - x : 0);
    return g.neg + 2 + (-x - 1) + nd;
}

// printf("%.6g", (double)f) into out (no terminator); returns the length (at most kMaxG)
WS_TEXT_FN int g6_write(const G6 &g, char *out)
{
    int n = 0;
    if (g.neg) out[n++] = '-';
    if (g.kind == 1) { out[n++] = '0'; return n; }
    if (g.kind == 2) { out[n++] = 'i'; out[n++] = 'n'; out[n++] = 'f'; return n; }
    if (g.kind == 3) { out[n++] = 'n'; out[n++] = 'a'; out[n++] = 'n'; return n; }
    const int nd = g6_sig_digits(g.digits), x = g.exp10;
    uint32_t d = g.digits, div = 100000u;
    if (x < -4 || x >= 6) {
        for (int i = 0; i < nd; ++i) {
            out[n++] = (char)('0' + d / div);
            d %= div;
            div /= 10u;
            if (i == 0 && nd > 1) out[n++] = '.';
        }
        out[n++] = 'e';
        out[n++] = x < 0 ? '-' : '+';
        const int ax = x < 0 ? -x : x;
        if (ax >= 100) out[n++] = (char)('0' + ax / 100);
        out[n++] = (char)('0' + ax / 10 % 10);
        out[n++] = (char)('0' + ax % 10);
        return n;
    }
    if (x < 0) {
        out[n++] = '0';
        out[n++] = '.';
        for (int i = 0; i < -x - 1; ++i) out[n++] = '0';
    }
    const int whole = x >= 0 ? x + 1 : 0; // digits before the point
    const int last = nd > whole ? nd : whole;
    for (int i = 0; i < last; ++i) {
        if (i == whole && x >= 0) out[n++] = '.';
        out[n++] = (char)('0' + d / div);
        d %= div;
        div /= 10u;
    }
    return n;
}

WS_TEXT_FN int g_format(float f, char *out) { return g6_write(g6_decompose(f), out); }

// decimal text of an unsigned integer (the header's counts: uint64_t; colours and indices: uint32_t, which keeps the
// kernels off 64-bit division)
template <class U> WS_TEXT_FN int u_length(U v)
{
    int n = 1;
    while (v >= 10u) { v /= 10u; ++n; }
    return n;
}

template <class U> WS_TEXT_FN int u_format(U v, char *out)
{
    const int n = u_length(v);
    for (int i = n - 1; i >= 0; --i) { out[i] = (char)('0' + v % 10u); v /= 10u; }
    return n;
}

} // namespace text
} // namespace wsamd
