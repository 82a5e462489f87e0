// svr_chain.hpp -- exact replay of the ray caster's sample-parameter chain, shared by k_raycast (svr_raycast.hip) and the
// one-lane march of k_project and k_hits (svr_march.hpp); svr_selftest.hip checks these very functions against a plain loop
// (k_chain_selftest).
#pragma once
#include "svr_math.hpp"

namespace svr {

// ------------------------------------------------------------------------------------------------------------------
// The reference's sample parameters are a float accumulation chain t_{n+1} = fl(t_n + h) (raycasting.cu:63).  To skip
// samples without evaluating them the chain has to be replayed exactly.  Within one binade [2^e, 2^(e+1)) every t is
// a multiple of u = ulp, and fl(t + h) = t + delta with ONE delta for the whole binade (h = q u + r rounds to q u or
// (q + 1) u, the same way for every t, unless r is exactly u / 2 where ties-to-even alternates).  So k steps inside a
// binade are t + k * delta, computed on the integer mantissas; the step that crosses into the next binade is taken
// with a real float addition.  Chains the closed form does not cover (t < 1, a tie, delta == 0) are simply not
// skipped: the caller falls back to one chunk at a time.
// ------------------------------------------------------------------------------------------------------------------
struct ChainSeg { uint32_t A, J, kmax; float u; bool ok; };     // t = A u, delta = J u, steps k <= kmax stay in the binade

SVR_DEV ChainSeg chain_segment(float t, float h)
{
    ChainSeg g;
    const uint32_t tb = __float_as_uint(t);
    const uint32_t ex = tb >> 23;                                   // t >= 1: sign 0, exponent >= 127
    g.u = __uint_as_float((ex - 23u) << 23);
    g.A = (tb & 0x7fffffu) | 0x800000u;
    const float t1 = t + h;
    const float delta = t1 - t;                                     // exact
    const float err = h - delta;                                    // exact: the rounding error of t + h
    const bool same = (__float_as_uint(t1) >> 23) == ex;
    g.J = (uint32_t)(delta * __uint_as_float((127u + 127u + 23u - ex) << 23));        // delta / u, an integer < 2^24
    g.ok = same && delta > 0.f && __builtin_fabsf(err) != 0.5f * g.u && t >= 1.f && ex < 127u + 100u;
    g.kmax = g.ok ? (0xffffffu - g.A) / g.J : 0u;
    return g;
}

// number of chain elements t^[0] = t, t^[1], ... that are < bound (inclusive: <= bound); exact = false if the chain left
// the closed form before the answer was known (then the count is a lower bound that is still safe to skip)
SVR_DEV uint32_t chain_count(float t, float h, float bound, bool inclusive, bool& exact)
{
    uint32_t n = 0;
    exact = true;
    for (int seg = 0; seg < 6; ++seg) {
        if (!(inclusive ? t <= bound : t < bound)) return n;
        const ChainSeg g = chain_segment(t, h);
        if (!g.ok) {
            // one real step (binade crossing) -- or give up on anything the closed form does not cover
            const float t1 = t + h;
            if (!(t1 > t) || !(t >= 1.f)) { exact = false; return n; }
            n += 1u; t = t1;
            continue;
        }
        // elements t + k delta, k = 0 .. kmax, of this binade that are before the bound
        const float xs = bound * __uint_as_float((254u - (__float_as_uint(g.u) >> 23)) << 23);      // bound / u (exact scaling)
        uint32_t k_in;
        if (xs >= 16777216.f) k_in = g.kmax + 1u;                  // the bound lies beyond this binade
        else {
            const float fl = __builtin_floorf(xs);
            uint32_t X = (uint32_t)fl;                               // t is before the bound, so X >= A >= 2^23
            if (!inclusive && fl == xs) X -= 1u;                   // strict: A + k J <= ceil(x) - 1
            k_in = X >= g.A ? (X - g.A) / g.J + 1u : 0u;
            if (k_in > g.kmax + 1u) k_in = g.kmax + 1u;
        }
        n += k_in;
        if (k_in <= g.kmax) return n;                              // the bound was met inside the binade
        // all kmax + 1 elements counted: continue from the first element of the next binade
        t = (float)(g.A + g.kmax * g.J) * g.u;
        t = t + h;
    }
    exact = false;
    return n;
}

// t after n chain steps; ok = false if the closed form gave up (t is then unchanged)
SVR_DEV float chain_advance(float t, float h, uint32_t n, bool& ok)
{
    const float t_in = t;
    ok = true;
    for (int seg = 0; seg < 8 && n != 0u; ++seg) {
        const ChainSeg g = chain_segment(t, h);
        if (!g.ok) {
            const float t1 = t + h;
            if (!(t1 > t) || !(t >= 1.f)) { ok = false; return t_in; }
            t = t1; n -= 1u;
            continue;
        }
        const uint32_t k = n < g.kmax ? n : g.kmax;
        t = (float)(g.A + k * g.J) * g.u;                          // exact: an integer below 2^24 times a power of two
        n -= k;
        if (n != 0u) { t = t + h; n -= 1u; }                       // the crossing step
    }
    if (n != 0u) { ok = false; return t_in; }
    return t;
}

} // namespace svr
