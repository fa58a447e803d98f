// Operand layout of v_smfmac_f32_16x16x64_f16 on gfx950, checked against what csrc/mfma_sparse_tiles.h assumes:
//   B (64 x 16): lane (col = lane & 15, g = lane >> 4), 8 registers of two halves; registers 2t, 2t+1 are one group of four k;
//   A (16 x 64 at 2:4): lane (row = lane & 15, kg = lane >> 4) holds 8 kept values; its values 2p, 2p+1 are the kept pair
//     of the group of four that B holds in lane group 2 (kg & 1) + (p >> 1), registers 2t, 2t+1 with t = 2 (kg >> 1) + (p & 1),
//     and the low 16 bits of the index register hold their positions in it: bits [4p+1:4p] and [4p+3:4p+2];
//   D (16 x 16): lane (col = lane & 15, g = lane >> 4) holds rows 4 g .. 4 g + 3.
// (Only this pairing matters to the kernel, not which k of the instruction's own numbering a register is.)
// A random 2:4 matrix of small integers times a random B, against the host product (exact in float16 / float32); then, for
// reading the layout off if that fails, D for B = one row of ones at a time (which k each kept value of row 0 multiplies).
//   hipcc -O2 --offload-arch=gfx950 smfmac_layout.hip -o smfmac_layout && ./smfmac_layout
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef _Float16 h16v __attribute__((ext_vector_type(16)));
typedef float f4v __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(64) void probe(const _Float16* a, const _Float16* b, const int* idx, float* d) {
  const int lane = threadIdx.x;
  h8v av;
  h16v bv;
  for (int j = 0; j < 8; ++j) av[j] = a[lane * 8 + j];
  for (int j = 0; j < 16; ++j) bv[j] = b[lane * 16 + j];
  f4v acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_smfmac_f32_16x16x64_f16(av, bv, acc, idx[lane], 0, 0);
  for (int i = 0; i < 4; ++i) d[lane * 4 + i] = acc[i];
}

static void run(const _Float16* a, const _Float16* b, const int* idx, float* d, void* dev[4]) {
  (void)hipMemcpy(dev[0], a, 64 * 8 * sizeof(_Float16), hipMemcpyHostToDevice);
  (void)hipMemcpy(dev[1], b, 64 * 16 * sizeof(_Float16), hipMemcpyHostToDevice);
  (void)hipMemcpy(dev[2], idx, 64 * sizeof(int), hipMemcpyHostToDevice);
  hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, (const _Float16*)dev[0], (const _Float16*)dev[1], (const int*)dev[2], (float*)dev[3]);
  (void)hipMemcpy(d, dev[3], 64 * 4 * sizeof(float), hipMemcpyDeviceToHost);
}

int main() {
  void* dev[4];
  const size_t bytes[4] = {64 * 8 * sizeof(_Float16), 64 * 16 * sizeof(_Float16), 64 * sizeof(int), 64 * 4 * sizeof(float)};
  for (int i = 0; i < 4; ++i)
    if (hipMalloc(&dev[i], bytes[i]) != hipSuccess) return 1;
  static _Float16 a[64 * 8], b[64 * 16];
  static int idx[64];
  static float d[64 * 4], A[16][64], B[64][16];
  srand(1);
  for (int lane = 0; lane < 64; ++lane) idx[lane] = 0;
  for (int row = 0; row < 16; ++row)
    for (int grp = 0; grp < 16; ++grp) {
      int i0 = rand() % 3, i1 = i0 + 1 + rand() % (3 - i0);
      for (int pos = 0; pos < 4; ++pos) A[row][4 * grp + pos] = 0.f;
      A[row][4 * grp + i0] = (float)(1 + rand() % 7);
      A[row][4 * grp + i1] = -(float)(1 + rand() % 7);
      const int gb = grp >> 2, t = grp & 3;        // the group of four as B holds it: lane group gb, registers 2t, 2t+1
      const int lane = row + 16 * ((gb >> 1) + 2 * (t >> 1)), p = 2 * (gb & 1) + (t & 1);
      a[lane * 8 + 2 * p] = (_Float16)A[row][4 * grp + i0];
      a[lane * 8 + 2 * p + 1] = (_Float16)A[row][4 * grp + i1];
      idx[lane] |= (i0 | (i1 << 2)) << (4 * p);
    }
  for (int k = 0; k < 64; ++k)
    for (int col = 0; col < 16; ++col) {
      B[k][col] = (float)(rand() % 9 - 4);
      b[(col + 16 * (k >> 4)) * 16 + (k & 15)] = (_Float16)B[k][col];
    }
  run(a, b, idx, d, dev);
  int bad = 0;
  for (int row = 0; row < 16; ++row)
    for (int col = 0; col < 16; ++col) {
      float want = 0.f;
      for (int k = 0; k < 64; ++k) want += A[row][k] * B[k][col];
      const float got = d[(col + 16 * (row >> 2)) * 4 + (row & 3)];
      if (got != want) ++bad;
    }
  printf("random 2:4 product against the host: %d of 256 entries differ -> the assumed layout is %s\n", bad, bad ? "WRONG" : "right");
  // which k does each kept value multiply?  kept value c' (= 8 kg + j) of every row is c' + 1; B = ones in row k only
  // (k = 16 g + 2 m + s: half s of register m of lane group g)
  for (int pat = 0; pat < 2; ++pat) {
    for (int lane = 0; lane < 64; ++lane) {
      for (int j = 0; j < 8; ++j) a[lane * 8 + j] = (_Float16)(float)(8 * (lane >> 4) + j + 1);
      idx[lane] = pat == 0 ? 0x4444 : 0xe9e9;      // positions (0, 1) in every group; (1, 2) and (2, 3) alternating
    }
    printf("positions %s: k -> kept value of row 0 that multiplies it (0: none)\n ", pat == 0 ? "(0,1) everywhere" : "(1,2),(2,3) alternating");
    for (int k = 0; k < 64; ++k) {
      for (int i = 0; i < 64 * 16; ++i) b[i] = (_Float16)0.f;
      for (int col = 0; col < 16; ++col) b[(col + 16 * (k >> 4)) * 16 + (k & 15)] = (_Float16)1.f;
      run(a, b, idx, d, dev);
      printf(" %d", (int)d[0]);
    }
    printf("\n");
  }
  return bad != 0;
}
