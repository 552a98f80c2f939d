// R1CS over the any-modulus path (device/r1cs_generic_kernels.hpp): the row kernel in the instantiation classes of the
// replay (kernels_generic.hip) -- up to eight words of characteristic with the word counts at compile time, then the
// capacity classes 16 / 32 / 64 / 128 words -- and the quotient kernel per capacity class.
#include <vector>

#define ZKGPU_GENERIC_NO_DUMP   // (dump_generic_kernel is kernels_generic.hip's)
#include "device/r1cs_generic_kernels.hpp"

namespace zkgpu {

template <bool ASSIGN>
static void launch_rows(dim3 grid, hipStream_t st, const R1csArgs& a, const GenericParams* gp, u32 nwords, u32 k_words) {
  switch (k_words <= 8 ? k_words : 0) {
    case 1: r1cs_generic_row_kernel<8, 1, ASSIGN><<<grid, 256, 0, st>>>(a, gp); return;
    case 2: r1cs_generic_row_kernel<8, 2, ASSIGN><<<grid, 256, 0, st>>>(a, gp); return;
    case 3: r1cs_generic_row_kernel<8, 3, ASSIGN><<<grid, 256, 0, st>>>(a, gp); return;
    case 4: r1cs_generic_row_kernel<8, 4, ASSIGN><<<grid, 256, 0, st>>>(a, gp); return;
    case 5: r1cs_generic_row_kernel<8, 5, ASSIGN><<<grid, 256, 0, st>>>(a, gp); return;
    case 6: r1cs_generic_row_kernel<8, 6, ASSIGN><<<grid, 256, 0, st>>>(a, gp); return;
    case 7: r1cs_generic_row_kernel<8, 7, ASSIGN><<<grid, 256, 0, st>>>(a, gp); return;
    case 8: r1cs_generic_row_kernel<8, 8, ASSIGN><<<grid, 256, 0, st>>>(a, gp); return;
    default: break;
  }
  if (nwords <= 16) r1cs_generic_row_kernel<16, 0, ASSIGN><<<grid, 256, 0, st>>>(a, gp);
  else if (nwords <= 32) r1cs_generic_row_kernel<32, 0, ASSIGN><<<grid, 256, 0, st>>>(a, gp);
  else if (nwords <= 64) r1cs_generic_row_kernel<64, 0, ASSIGN><<<grid, 256, 0, st>>>(a, gp);
  else r1cs_generic_row_kernel<kGenericMaxWords, 0, ASSIGN><<<grid, 256, 0, st>>>(a, gp);
}

void launch_r1cs_generic(bool assign, dim3 grid, hipStream_t st, const R1csArgs& a, const GenericParams* gp, u32 nwords, u32 k_words) {
  if (assign) launch_rows<true>(grid, st, a, gp, nwords, k_words);
  else launch_rows<false>(grid, st, a, gp, nwords, k_words);
}

void launch_r1cs_corr_generic(dim3 grid, hipStream_t st, const R1csCorrArgs& a, const GenericParams* gp, const GenericCorrParams* cp,
                              u32 nwords) {
  if (nwords <= 8) r1cs_generic_correction_kernel<8><<<grid, 256, 0, st>>>(a, gp, cp);
  else if (nwords <= 16) r1cs_generic_correction_kernel<16><<<grid, 256, 0, st>>>(a, gp, cp);
  else if (nwords <= 32) r1cs_generic_correction_kernel<32><<<grid, 256, 0, st>>>(a, gp, cp);
  else if (nwords <= 64) r1cs_generic_correction_kernel<64><<<grid, 256, 0, st>>>(a, gp, cp);
  else r1cs_generic_correction_kernel<kGenericMaxWords><<<grid, 256, 0, st>>>(a, gp, cp);
}

// p = 2^shift * m, m odd; m^{-1} mod 2^(32 nwords) by Hensel lifting from the inverse mod 2^32: x <- x * (2 - m * x)
void generic_quotient_params(const GenericParams* gp, GenericCorrParams* cp) {
  const u32 n = gp->nwords;
  *cp = GenericCorrParams{};
  u32 s = 0;
  while (s < 32 * gp->k && !(gp->p[s / 32] >> (s % 32) & 1)) ++s;
  cp->shift = s;
  std::vector<u32> m(n, 0), x(n, 0), t(n), u(n);
  for (u32 i = 0; i < n; ++i) {   // m = p >> s
    const u32 lo = i + s / 32 < gp->k ? gp->p[i + s / 32] : 0u, hi = i + s / 32 + 1 < gp->k ? gp->p[i + s / 32 + 1] : 0u;
    m[i] = s % 32 ? (lo >> (s % 32)) | (hi << (32 - s % 32)) : lo;
  }
  u32 inv = 1;
  for (int i = 0; i < 5; ++i) inv *= 2 - m[0] * inv;
  x[0] = inv;
  for (u32 bits = 32; bits < 32 * n; bits *= 2) {
    g_mul_low(m.data(), x.data(), t.data(), n);   // m * x
    u32 borrow = 0;                               // 2 - m * x
    for (u32 i = 0; i < n; ++i) {
      const u64 d = (u64)(i == 0 ? 2u : 0u) - t[i] - borrow;
      u[i] = (u32)d;
      borrow = (u32)(d >> 63);
    }
    g_mul_low(x.data(), u.data(), t.data(), n);
    x = t;
  }
  for (u32 i = 0; i < n; ++i) cp->minv[i] = x[i];
}

int r1cs_generic_selftest(const GenericParams* gp, int op, u32 n_terms, const u32* x, const u32* y, const u32* z, u32* out) {
  constexpr int CAP = kGenericMaxWords;
  if (gp->k == 0 || gp->k > (u32)CAP || gp->nwords > (u32)CAP || gp->nwords < gp->k) return 1;
  const u32 n = gp->nwords;
  switch (op) {
    case 0:
    case 1:
      if (n_terms == 0)
        for (u32 i = 0; i < n; ++i) out[i] = 0;
      for (u32 t = 0; t < n_terms; ++t) g_lincomb_step<CAP>(out, x + (size_t)t * n, op == 0 ? y + (size_t)t * n : nullptr, t == 0, gp);
      return 0;
    case 2:
    case 3: {
      GenericCorrParams cp;
      generic_quotient_params(gp, &cp);
      g_exact_quotient<CAP>(x, y, z, op == 3, &cp, out, gp);
      return 0;
    }
    default: return 1;
  }
}

}  // namespace zkgpu
