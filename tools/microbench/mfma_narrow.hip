// Round 5: what does v_mfma_f32_16x16x16_f16 cost on gfx950 next to v_mfma_f32_16x16x32_f16 --
// alone (pipe cycles) and between the vector mix of fista_mfma_kernel (issue-port hold)?  If the narrow instruction ran
// in <= 0.6 of the wide one's time, the block products of the kernel could skip the empty quarter of the diagonal tile
// and the constant quarter of the previous-block tile (6 narrow products instead of 4 wide per split product).
// Also: v_mfma_f32_32x32x16_f16 and the 4x4x4 (64 blocks) form, for completeness.
// And v_smfmac_f32_16x16x64_f16 (A 16x64 at 2:4 sparsity, B dense 64x16): one of them could carry both near tiles of a
// block of fista_mfma_kernel (120 matrix instructions per iteration instead of 228, ~8.3 vector instructions per gap).
// The last lines apply the issue model n_m*p_m + n_v*p_v to the measured prices (gate of the sparse-tile kernel).
//   hipcc -O3 --offload-arch=gfx950 mfma_narrow.hip -o mfma_narrow && ./mfma_narrow
#include <hip/hip_runtime.h>
#include <cstdio>

constexpr int ITERS = 16384;      // (long launches, and a warm-up before the first measurement: short ones run at idle clocks)
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));
typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef _Float16 h4v __attribute__((ext_vector_type(4)));
typedef _Float16 h16v __attribute__((ext_vector_type(16)));

// MK: 1 = 16x16x32 f16 (8 halves per lane), 2 = 16x16x16 f16 (4 halves per lane), 3 = 32x32x8 f16 (4 halves), 4 = 32x32x16 f16 (8 halves)
//     5 = sparse 16x16x64 f16 (A: 8 compressed halves + one index register, B: 16 halves per lane)
// NV vector instructions (the kernel's mix) after every matrix instruction; NCH independent accumulator chains
template <int MK, int NV, int NCH>
__global__ __launch_bounds__(256) void k(float* out, float a, float b, int iters) {
  h8v ha8, hb8;
  h4v ha4, hb4;
  h16v hb16;
  for (int i = 0; i < 16; ++i) hb16[i] = (_Float16)(b * (i & 7));
  int sidx = 0x4e4e + (int)a;      // (2-bit positions of the kept pair in each group of four; any value times the same)
  asm volatile("" : "+v"(sidx));
  for (int i = 0; i < 8; ++i) { ha8[i] = (_Float16)(a + i); hb8[i] = (_Float16)(b * i); }
  for (int i = 0; i < 4; ++i) { ha4[i] = (_Float16)(a + i); hb4[i] = (_Float16)(b * i); }
  f4v c4[8] = {};
  f16v c16[2] = {};
  double dac[4] = {a, b, a + b, a - b};
  float cf[4] = {a, b, a + b, a - b};
  const double da = a, db = b;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      // (inline asm on VGPR operands: the builtins put C/D into the accumulator file and shuffle it around the loop)
      if constexpr (MK == 1) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(c4[g % NCH]) : "v"(ha8), "v"(hb8));
      if constexpr (MK == 2) asm volatile("v_mfma_f32_16x16x16_f16 %0, %1, %2, %0" : "+v"(c4[g % NCH]) : "v"(ha4), "v"(hb4));
      if constexpr (MK == 3) asm volatile("v_mfma_f32_32x32x8_f16 %0, %1, %2, %0" : "+v"(c16[g % 2]) : "v"(ha4), "v"(hb4));
      if constexpr (MK == 4) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(c16[g % 2]) : "v"(ha8), "v"(hb8));
      if constexpr (MK == 5) asm volatile("v_smfmac_f32_16x16x64_f16 %0, %1, %2, %3" : "+v"(c4[g % NCH]) : "v"(ha8), "v"(hb16), "v"(sidx));
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        const int i = (g * NV + u) & 3, kind = (g * NV + u) % 5;
        if (kind == 0) asm volatile("v_fma_f64 %0, %1, %2, %0" : "+v"(dac[i]) : "v"(da), "v"(db));
        if (kind == 1) asm volatile("v_max_f64 %0, %1, %0" : "+v"(dac[i]) : "v"(da));
        if (kind == 2) asm volatile("v_cvt_f32_f64 %0, %1" : "=v"(cf[i]) : "v"(dac[i]));
        if (kind == 3) { int pk; asm volatile("v_cvt_pkrtz_f16_f32 %0, %1, %2" : "=v"(pk) : "v"(cf[i]), "v"(cf[(i + 1) & 3])); asm volatile("" :: "v"(pk)); }
        if (kind == 4) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(cf[i]) : "v"(a), "v"(b));
      }
    }
  }
  float s = 0;
  for (int i = 0; i < 8; ++i) s += c4[i][0] + c4[i][3];
  for (int i = 0; i < 4; ++i) s += (float)dac[i] + cf[i];
  for (int i = 0; i < 16; ++i) s += c16[0][i] + c16[1][i];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <typename F>
float run(F launch) {
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  for (int w = 0; w < 12; ++w) launch();
  hipDeviceSynchronize();
  float best = 1e30f;
  for (int r = 0; r < 5; ++r) {
    hipEventRecord(e0);
    launch();
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    if (ms < best) best = ms;
  }
  return best;
}

int main() {
  float* out;
  if (hipMalloc(&out, 256 * 4 * 2 * 256 * sizeof(float) * 4) != hipSuccess) return 1;
  int clk = 0;
  hipDeviceGetAttribute(&clk, hipDeviceAttributeClockRate, 0);
  for (int wps = 1; wps <= 2; ++wps) {
  printf("%d wave(s) per SIMD, %d trips x 8 matrix instructions; ms per launch (best of 5) and ns per matrix instruction [+ its vector instructions] and wave\n", wps, ITERS);
  float ns_last = 0;
#define T(MK, NV, NCH, label) { float ms = run([&] { hipLaunchKernelGGL((k<MK, NV, NCH>), dim3(256 * wps), dim3(256), 0, 0, out, 1.0f, 0.5f, ITERS); }); \
    printf("  %-72s %8.3f ms  %7.2f ns\n", label, ms, ms * 1e6 / (ITERS * 8.0 * wps)); ns_last = ms * 1e6 / (ITERS * 8.0 * wps); }
  T(1, 0, 4, "16x16x32 f16, 4 chains");
  T(1, 0, 2, "16x16x32 f16, 2 chains");
  T(1, 0, 1, "16x16x32 f16, 1 chain (dependent)");
  T(2, 0, 4, "16x16x16 f16, 4 chains");
  T(2, 0, 2, "16x16x16 f16, 2 chains");
  T(2, 0, 1, "16x16x16 f16, 1 chain (dependent)");
  T(3, 0, 2, "32x32x8 f16, 2 chains");
  T(4, 0, 2, "32x32x16 f16, 2 chains");
  T(1, 2, 2, "16x16x32 f16 + 2 vector");
  T(1, 4, 2, "16x16x32 f16 + 4 vector       (~ fista_mfma_kernel: 4.4 vector per matrix instruction)");
  T(1, 4, 1, "16x16x32 f16 + 4 vector, ONE accumulator chain (each product waits for the one before)");
  T(1, 4, 4, "16x16x32 f16 + 4 vector, four chains");
  T(1, 5, 2, "16x16x32 f16 + 5 vector");
  T(1, 5, 1, "16x16x32 f16 + 5 vector, one chain");
  T(1, 6, 2, "16x16x32 f16 + 6 vector");
  T(0, 4, 2, "4 vector alone");
  T(0, 6, 2, "6 vector alone");
  T(4, 8, 2, "32x32x16 f16 + 8 vector       (the same work as 2 x (16x16x32 + 4 vector))");
  T(4, 10, 2, "32x32x16 f16 + 10 vector");
  T(2, 2, 2, "16x16x16 f16 + 2 vector");
  T(2, 3, 2, "16x16x16 f16 + 3 vector       (6 narrow for 4 wide: 2.9 vector per matrix instruction)");
  T(2, 4, 2, "16x16x16 f16 + 4 vector");
  T(2, 6, 2, "16x16x16 f16 + 6 vector");
  // the sparse instruction, and the dense one again next to it (same launch sequence, same clocks)
  T(5, 0, 4, "sparse 16x16x64 f16, 4 chains");                                          const float s0 = ns_last;
  T(5, 0, 1, "sparse 16x16x64 f16, 1 chain (dependent)");
  T(5, 4, 2, "sparse 16x16x64 f16 + 4 vector");                                         const float s4 = ns_last;
  T(5, 8, 2, "sparse 16x16x64 f16 + 8 vector    (~ the sparse-tile kernel: 8.3 vector per matrix instruction)"); const float s8 = ns_last;
  T(5, 9, 2, "sparse 16x16x64 f16 + 9 vector");                                         const float s9 = ns_last;
  T(1, 0, 4, "16x16x32 f16, 4 chains (again)");                                         const float d0 = ns_last;
  T(1, 4, 2, "16x16x32 f16 + 4 vector (again)");                                        const float d4 = ns_last;
  T(1, 5, 2, "16x16x32 f16 + 5 vector (again)");                                        const float d5 = ns_last;
  T(0, 4, 2, "4 vector alone (again)");                                                 const float v4 = ns_last;
  T(0, 8, 2, "8 vector alone");                                                         const float v8 = ns_last;
  T(0, 9, 2, "9 vector alone");                                                         const float v9 = ns_last;
  {
    // issue model of fista_mfma_kernel's iteration: n_m * p_m + n_v * p_v, p_v from the vector-only rows, p_m = what the
    // matrix instruction adds to its gap's vector instructions; dense 228 + 996, sparse 120 + 996 (8.3 per gap: between the
    // + 8 and + 9 rows).  Second form: whole gaps, interpolated between the measured rows, with no additivity assumed.
    const float pv = (v8 / 8 + v9 / 9 + v4 / 4) / 3;
    const float pmd = 0.5f * ((d4 - v4) + (d5 - (v4 + (v8 - v4) / 4)));
    const float pms = 0.5f * ((s8 - v8) + (s9 - v9));
    const float dense = 228 * pmd + 996 * pv, sparse = 120 * pms + 996 * pv;
    const float gd = 996.0f / 228 - 4, gs = 996.0f / 120 - 8;
    const float dense_g = 228 * (d4 + gd * (d5 - d4)), sparse_g = 120 * (s8 + gs * (s9 - s8));
    printf("  model, additive: p_v %.3f ns, p_m dense %.3f ns, p_m sparse %.3f ns (alone: dense %.2f, sparse %.2f; sparse + 4: %.2f)\n", pv, pmd, pms, d0, s0, s4);
    printf("  model, additive: dense 228 x p_m + 996 x p_v = %.1f ns, sparse 120 x p_m + 996 x p_v = %.1f ns, sparse / dense = %.4f\n", dense, sparse, sparse / dense);
    printf("  model, whole gaps: dense 228 x gap(4.37) = %.1f ns, sparse 120 x gap(8.30) = %.1f ns, sparse / dense = %.4f\n", dense_g, sparse_g, sparse_g / dense_g);
  }
  }
  return 0;
}
