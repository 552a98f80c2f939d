// R1CS over the any-modulus path: the row kernel and the quotient ("correction") kernel for the fields whose wires hold
// canonical residues (generic_kernels.hpp: even characteristics, the rings Z / 2^B, characteristics wider than 512 bits).
//
// The reference's ToR1CSConverter works on BigUint (rust/src/consumers/to_r1cs.rs:93-393): it converts a relation over
// any modulus.  These kernels are r1cs_row_kernel / r1cs_correction_kernel (r1cs_kernels.hpp) with the arithmetic of
// generic_kernels.hpp: same row and term encoding (R1csRow / R1csTerm), same wire table layout with a run time chunk
// count, one wave per row (or call) x 64 witnesses.  The coefficient pool holds canonical words; every combination is of
// class full (the unit / small classes are a Montgomery-path trick).
//
// Reduction of a combination: one Barrett reduction per product (g_mul) and one conditional subtraction per addition
// (g_add), so that every partial sum is canonical.  A lazier sum would have to stay below 2^(64 k), the precondition of
// HAC 14.42 (g_barrett); 255 products of (p - 1)^2 do not.  Powers of two take the low bits and let sums wrap.
//
// The arithmetic is plain C++ on 32-bit words (`__host__ __device__`): the CPU tier runs it against Python integers
// through zkgpu_r1cs_generic_selftest (capi.cpp).
#pragma once
#include "generic_kernels.hpp"
#include "r1cs_kernels.hpp"

namespace zkgpu {

// One step of a combination: acc = acc + c * v mod p, or acc = c * v for the first term; c == nullptr: coefficient 1.
// v and c canonical (n = nwords words each), acc canonical after every step.
template <int CAP, class P>
ZKGPU_HD void g_lincomb_step(u32* acc, const u32* v, const u32* c, bool first, const P* gp) {
  const u32 n = gp->nwords;
  u32 t[CAP];
  if (c) g_mul<CAP>(v, c, t, gp);
  else
    for (u32 i = 0; i < n; ++i) t[i] = v[i];
  if (first)
    for (u32 i = 0; i < n; ++i) acc[i] = t[i];
  else
    g_add<CAP>(acc, t, acc, gp);
}

// r = a * b mod 2^(32 n) (r must not alias a or b)
ZKGPU_HD void g_mul_low(const u32* a, const u32* b, u32* r, u32 n) {
  GAcc acc{0, 0};
  for (u32 col = 0; col < n; ++col) {
    for (u32 i = 0; i <= col; ++i) acc.mac(a[i], b[col - i]);
    r[col] = acc.shift();
  }
}

// The quotient wire of a call (to_r1cs.rs:163-211, :213-260, :262-359): q = (a op b - out) / p, an exact division
// with q < 2^(32 n) (a, out < p; b < p or a raw constant below 2^(32 n)).  With p = 2^s * m, m odd:
//     q = ((a op b - out) >> s) * m^{-1}  mod 2^(32 n)
// The difference is formed over W = n + ceil(s / 32) words: bits s .. s + 32 n of it are the ones the shift keeps.
// A power of two has m = 1.  (s and m^{-1}: GenericCorrParams, filled on the host by generic_quotient_params.)
template <int CAP, class P>
ZKGPU_HD void g_exact_quotient(const u32* a, const u32* b, const u32* out, bool mul, const GenericCorrParams* cp, u32* q,
                               const P* gp) {
  const u32 n = gp->nwords, s = cp->shift, sw = s / 32, sb = s % 32, W = n + (s + 31) / 32;   // W <= 2 n: s < 32 k
  u32 d[2 * CAP];
  if (mul) {
    GAcc acc{0, 0};
    for (u32 col = 0; col < W; ++col) {
      const u32 i_lo = col >= n ? col - (n - 1) : 0, i_hi = col < n ? col : n - 1;
      for (u32 i = i_lo; i <= i_hi; ++i) acc.mac(a[i], b[col - i]);
      d[col] = acc.shift();
    }
  } else {
    u64 c = 0;
    for (u32 i = 0; i < W; ++i) {
      if (i < n) c += (u64)a[i] + b[i];
      d[i] = (u32)c;
      c >>= 32;
    }
  }
  u32 borrow = 0;
  for (u32 i = 0; i < W; ++i) {
    const u64 x = (u64)d[i] - (i < n ? out[i] : 0u) - borrow;
    d[i] = (u32)x;
    borrow = (u32)(x >> 63);
  }
  u32 e[CAP];   // the low n words of (a op b - out) >> s
  for (u32 i = 0; i < n; ++i) {
    const u32 lo = d[i + sw], hi = i + sw + 1 < W ? d[i + sw + 1] : 0u;
    e[i] = sb ? (lo >> sb) | (hi << (32 - sb)) : lo;
  }
  g_mul_low(e, cp->minv, q, n);
}

#ifdef __HIPCC__
// the parameters of a characteristic of KC words in registers (generic_kernels.hpp SmallParams): SGPRs up to six words;
// seven or eight words of p and mu in SGPRs made the row kernel spill SGPRs, so those are read through a pointer that
// the compiler cannot prove uniform (an offset of zero per lane) and land in VGPRs
template <int KC>
__device__ __forceinline__ SmallParams<KC> r1cs_small_params(const GenericParams* gp) {
  SmallParams<KC> sp;
  if constexpr (KC <= 6) {
    typedef const GenericParams __attribute__((address_space(4))) GpS;
    GpS* g = (GpS*)(unsigned long long)gp;
#pragma unroll
    for (int i = 0; i < KC; ++i) sp.p[i] = g->p[i];
#pragma unroll
    for (int i = 0; i < KC + 2; ++i) sp.mu[i] = g->mu[i];
    sp.pow2_bits = g->pow2_bits;
  } else {
    const u32 zero = threadIdx.x / blockDim.x;
    const GenericParams* g = gp + zero;
#pragma unroll
    for (int i = 0; i < KC; ++i) sp.p[i] = g->p[i];
#pragma unroll
    for (int i = 0; i < KC + 2; ++i) sp.mu[i] = g->mu[i];
    sp.pow2_bits = gp->pow2_bits;
  }
  return sp;
}

// entry `idx` of the canonical coefficient pool: vector loads of one address (the scalar path would hold eight more SGPRs
// per coefficient next to p and mu, and the eight-word instantiations spilled them)
__device__ __forceinline__ void r1cs_generic_coef(const u32* coefs, u32 idx, u32 n, u32* c) {
  const u32* q = coefs + (size_t)idx * n;
  for (u32 i = 0; i < n; ++i) c[i] = q[i];
}

// the value of a term: the wire, or canonical 1 (pool entry one_coef) for the constant one
__device__ __forceinline__ void r1cs_generic_value(const R1csArgs& args, const uint4* __restrict__ T, u32 rec, const R1csTerm e, u32 n,
                                                   u32* v) {
  if (e.slot == 0xFFFFFFFFu) r1cs_generic_coef(args.coefs, args.one_coef, n, v);
  else g_wire_load(T + (size_t)e.slot * rec, n, v);
}

// <terms t0 .. t0 + cnt, w> into acc, one term at a time (with the gathers of two terms issued together the eight-word
// instantiations held 20-30 more VGPRs and fell to three waves per SIMD)
template <int CAP, class P>
__device__ __forceinline__ void r1cs_generic_lincomb(const R1csArgs& args, const uint4* __restrict__ T, u32 rec, u32 t0, u32 cnt,
                                                     u32* acc, const P* gp) {
  const u32 n = gp->nwords;
  if (cnt == 0) {
    for (u32 i = 0; i < n; ++i) acc[i] = 0;
    return;
  }
  for (u32 t = t0; t < t0 + cnt; ++t) {
    const R1csTerm e = r1cs_load_term(args.terms, t);
    u32 v[CAP];
    r1cs_generic_value(args, T, rec, e, n, v);
    if (e.coef == 0xFFFFFFFFu) {
      g_lincomb_step<CAP>(acc, v, (const u32*)nullptr, t == t0, gp);
    } else {
      u32 c[CAP];
      r1cs_generic_coef(args.coefs, e.coef, n, c);
      g_lincomb_step<CAP>(acc, v, c, t == t0, gp);
    }
  }
}

// ASSIGN = false: compare <a,w> * <b,w> with <c,w> and record the first failing row per lane.
// ASSIGN = true : C is a single term with coefficient 1 (checked on the host); its slot receives <a,w> * <b,w>.
template <int CAP, bool ASSIGN, class P>
__device__ __forceinline__ void r1cs_generic_row_body(const R1csArgs& args, const P* gp) {
  const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const u32 lane = threadIdx.x & 63;
  const u32 lb = blockIdx.y;
  const u32 r = blockIdx.x * (blockDim.x >> 6) + wave;
  if (r >= args.n_rows) return;
  const u32 row = args.first_row + r;
  typedef const u32 __attribute__((address_space(4))) cu32;
  cu32* dq = (cu32*)(unsigned long long)(args.rows + __builtin_amdgcn_readfirstlane(row));
  const u32 first = dq[0], counts = dq[1];
  const u32 na = counts & 0xFF, nb = (counts >> 8) & 0xFF, nc = (counts >> 16) & 0xFF, flags = counts >> 24;
  const u32 n = gp->nwords;
  const u32 rec = ((n + 3) / 4) * 64;
  const uint4* __restrict__ T = args.table + (size_t)lb * args.n_slots * rec + lane;
  u32 prod[CAP], x[CAP];
  r1cs_generic_lincomb<CAP>(args, T, rec, first, na, prod, gp);
  if (!(flags & kR1csBIsOne)) {
    r1cs_generic_lincomb<CAP>(args, T, rec, first + na, nb, x, gp);
    g_mul<CAP>(prod, x, prod, gp);
  }
  if (ASSIGN) {
    const R1csTerm out = r1cs_load_term(args.terms, first + na + nb);
    uint4* __restrict__ O = args.table_out + (size_t)lb * args.n_slots * rec + lane;
    g_wire_store(O + (size_t)out.slot * rec, n, prod);
  } else {
    r1cs_generic_lincomb<CAP>(args, T, rec, first + na + nb, nc, x, gp);
    u32 diff = 0;
    for (u32 i = 0; i < n; ++i) diff |= prod[i] ^ x[i];
    const u32 lane_g = lb * 64 + lane;
    const bool bad = diff != 0 && lane_g < args.batch;
    if (__ballot(bad) != 0ull) {
      if (bad) atomicMin(&args.first_fail[lane_g], row);
    }
  }
}

// KC = 0: any characteristic of up to 32 CAP bits, the parameters read from memory; KC > 0: one of KC words, the word
// counts known at compile time (SmallParams: the operands stay in registers)
template <int CAP, int KC, bool ASSIGN>
__global__ __launch_bounds__(256) void r1cs_generic_row_kernel(const R1csArgs args, const GenericParams* gp) {
  if constexpr (KC == 0) {
    r1cs_generic_row_body<CAP, ASSIGN>(args, gp);
  } else {
    const SmallParams<KC> sp = r1cs_small_params<KC>(gp);
    r1cs_generic_row_body<CAP, ASSIGN>(args, &sp);
  }
}

// One wave = one call x 64 witnesses; the operands come out of the retain_all wire table (canonical already), the
// quotient goes out as nwords little-endian words per lane and call.  Stores: plain C++ (vector stores).
template <int CAP>
__global__ __launch_bounds__(256) void r1cs_generic_correction_kernel(const R1csCorrArgs args, const GenericParams* __restrict__ gp,
                                                                      const GenericCorrParams* __restrict__ cp) {
  const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const u32 lane = threadIdx.x & 63;
  const u32 lb = blockIdx.y;
  const u32 k = blockIdx.x * (blockDim.x >> 6) + wave;
  const u32 lane_g = lb * 64 + lane;
  if (k >= args.n_calls) return;
  const R1csCorrCall c = args.calls[k];
  const u32 n = gp->nwords;
  const u32 rec = ((n + 3) / 4) * 64;
  const uint4* __restrict__ T = args.table + (size_t)lb * args.n_slots * rec + lane;
  u32 a[CAP], b[CAP], o[CAP], q[CAP];
  g_wire_load(T + (size_t)c.a * rec, n, a);
  g_wire_load(T + (size_t)c.out * rec, n, o);
  if (c.flags & kCorrConstB) {   // the raw constant, as the call got it
    for (u32 i = 0; i < n; ++i) b[i] = args.consts[(size_t)c.b * n + i];
  } else {
    g_wire_load(T + (size_t)c.b * rec, n, b);
  }
  g_exact_quotient<CAP>(a, b, o, (c.flags & kCorrMul) != 0, cp, q, gp);
  if (lane_g < args.batch) {
    u32* dst = args.out + ((size_t)lane_g * args.n_calls + k) * n;
    for (u32 i = 0; i < n; ++i) dst[i] = q[i];
  }
}
#endif  // __HIPCC__

}  // namespace zkgpu
