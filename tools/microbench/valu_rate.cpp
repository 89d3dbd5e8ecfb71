// valu_rate -- issue cost of the FP64 / conversion / integer vector instructions the detect kernels are made of, in cycles per
// wavefront instruction per SIMD (development tool).  Eight independent chains per lane, 8 waves per SIMD, every SIMD of the device.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -x hip tools/microbench/valu_rate.cpp -o build_tmp/valu_rate && build_tmp/valu_rate
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#pragma clang diagnostic ignored "-Wunused-result"
#pragma clang diagnostic ignored "-Wunused-value"

template <int OP>
__global__ __launch_bounds__(256) void k(double* out, int iters, double seed) {
  double a[8];
  for (int q = 0; q < 8; q++) a[q] = seed + q * 0.37 + threadIdx.x * 1e-3;
  int ai[8];
  for (int q = 0; q < 8; q++) ai[q] = (int)a[q] + q;
  float af[8];
  for (int q = 0; q < 8; q++) af[q] = (float)a[q];
  unsigned long long au[8];
  for (int q = 0; q < 8; q++) au[q] = (unsigned long long)(a[q] * 1e6);
  const unsigned long long ub = (unsigned long long)out;
  const int sh = __builtin_amdgcn_readfirstlane(iters & 7);
  const double big = 0x1p52;
  int t32 = 0;
  for (int it = 0; it < iters; it++) {
#pragma unroll
    for (int q = 0; q < 8 && OP < 19; q++) {
      if (OP == 0) a[q] = a[q] + 1.25;                                   // v_add_f64
      if (OP == 1) a[q] = a[q] * 1.0000001;                              // v_mul_f64
      if (OP == 2) a[q] = __builtin_fma(a[q], 1.0000001, 0.5);           // v_fma_f64
      if (OP == 3) { ai[q] = (int)a[q]; a[q] += (double)0.0; asm volatile("" : "+v"(ai[q])); asm volatile("" : "+v"(a[q])); }   // v_cvt_i32_f64 (+ nothing)
      if (OP == 4) a[q] = __builtin_amdgcn_rcp(a[q]);                    // v_rcp_f64
      if (OP == 5) a[q] = 1.5 / a[q];                                    // full IEEE division
      if (OP == 6) a[q] = __builtin_sqrt(a[q]);                          // IEEE sqrt
      if (OP == 7) af[q] = af[q] * 1.0000001f + 0.5f;                    // f32 mul + add (no contraction)
      if (OP == 8) ai[q] = ai[q] * 3 + q;                                // integer mad
      if (OP == 9) { a[q] = (a[q] < 2.0) ? a[q] + 1.0 : a[q]; }          // compare + select (+ add)
      if (OP == 10) { ai[q] = __mul24(ai[q], 5) + 1; }
      // -- the rows below name their instruction in inline assembly: what is timed is what is written
      if (OP == 11) asm volatile("v_cvt_i32_f64 %0, %1" : "=v"(ai[q]) : "v"(a[q]));                                  // the conversion alone (row 3 adds a v_add_f64)
      if (OP == 12) asm volatile("v_lshl_add_u64 %0, %1, 2, %2" : "=v"(au[q]) : "v"(au[q]), "v"(ub));                // 64-bit address: base + (index << 2)
      if (OP == 13) asm volatile("v_add_lshl_u32 %0, %1, %2, 2" : "=v"(ai[q]) : "v"(ai[q]), "v"(iters));             // 32-bit byte offset: (row + col) << 2
      if (OP == 14) asm volatile("v_lshlrev_b64 %0, %1, %2" : "=v"(au[q]) : "s"(sh), "v"(au[q]));                    // 64-bit shift by a scalar
      if (OP == 15) asm volatile("v_cvt_f64_i32 %0, %1" : "=v"(a[q]) : "v"(ai[q]));
      if (OP == 16) asm volatile("v_cvt_f32_f64 %0, %1" : "=v"(af[q]) : "v"(a[q]));
      if (OP == 17) asm volatile("v_cndmask_b32 %0, 0, %1, vcc\n\tv_or_b32 %2, %2, %0" : "=&v"(t32) : "v"(iters), "v"(ai[q]) : "vcc");   // one mask bit: select + or
      if (OP == 18) asm volatile("v_add_f64 %0, %0, %1" : "+v"(a[q]) : "v"(big));                                     // the add of the sequences below, mode untouched
    }
    // x + 2^52 under round-toward-zero (low word = (int)x for 0 <= x < 2^31): one block = mode write, G adds, mode write back; the rows
    // report the block and its cost per add.  8 adds per line over the eight chains
#define RZ_ON "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 2, 2), 3\n\t"
#define RZ_OFF "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 2, 2), 0"
#define ADD1(r) "v_add_f64 %" #r ", %" #r ", %8\n\t"
#define ADD2(r, s) ADD1(r) ADD1(s)
#define ADD8 ADD2(0, 1) ADD2(2, 3) ADD2(4, 5) ADD2(6, 7)
#define CHAINS "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]) : "v"(big)
    if (OP == 19) {      // G = 2, four blocks
      asm volatile(RZ_ON ADD2(0, 1) RZ_OFF : CHAINS);
      asm volatile(RZ_ON ADD2(2, 3) RZ_OFF : CHAINS);
      asm volatile(RZ_ON ADD2(4, 5) RZ_OFF : CHAINS);
      asm volatile(RZ_ON ADD2(6, 7) RZ_OFF : CHAINS);
    }
    if (OP == 20) asm volatile(RZ_ON ADD8 ADD2(0, 1) ADD1(2) RZ_OFF : CHAINS);                 // G = 11
    if (OP == 21) asm volatile(RZ_ON ADD8 ADD8 ADD2(0, 1) ADD2(2, 3) ADD2(4, 5) RZ_OFF : CHAINS);   // G = 22
    {
    }
  }
  double s = 0;
  for (int q = 0; q < 8; q++) s += a[q] + ai[q] + af[q] + (double)au[q];
  s += t32;
  out[blockIdx.x * 256 + threadIdx.x] = s;
}

template <int OP>
double run(double* d, int iters) {
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  hipLaunchKernelGGL(k<OP>, dim3(256 * 8), dim3(256), 0, 0, d, 10, 1.5);
  hipEventRecord(e0, 0);
  hipLaunchKernelGGL(k<OP>, dim3(256 * 8), dim3(256), 0, 0, d, iters, 1.5);
  hipEventRecord(e1, 0);
  hipEventSynchronize(e1);
  float ms = 0; hipEventElapsedTime(&ms, e0, e1);
  return ms;
}

int main() {
  double* d; hipMalloc(&d, 256 * 8 * 256 * 8);
  int clk_khz = 0; hipDeviceGetAttribute(&clk_khz, hipDeviceAttributeClockRate, 0);
  const int iters = 4000;
  const char* names[] = {"v_add_f64", "v_mul_f64", "v_fma_f64", "v_cvt_i32_f64 + v_add_f64", "v_rcp_f64", "f64 division (IEEE)", "f64 sqrt (IEEE)", "f32 mul + add", "i32 mul + add", "f64 cmp + cndmask x2 + add", "mul24 + add",
                         "v_cvt_i32_f64", "v_lshl_add_u64", "v_add_lshl_u32", "v_lshlrev_b64 (scalar shift)", "v_cvt_f64_i32", "v_cvt_f32_f64", "v_cndmask_b32 + v_or_b32", "v_add_f64 (asm)",
                         "rtz: setreg, 2 adds, setreg", "rtz: setreg, 11 adds, setreg", "rtz: setreg, 22 adds, setreg"};
  constexpr int NOPS = 22;
  double ms[NOPS] = {run<0>(d, iters), run<1>(d, iters), run<2>(d, iters), run<3>(d, iters), run<4>(d, iters), run<5>(d, iters), run<6>(d, iters), run<7>(d, iters), run<8>(d, iters), run<9>(d, iters), run<10>(d, iters),
                     run<11>(d, iters), run<12>(d, iters), run<13>(d, iters), run<14>(d, iters), run<15>(d, iters), run<16>(d, iters), run<17>(d, iters), run<18>(d, iters), run<19>(d, iters), run<20>(d, iters), run<21>(d, iters)};
  // (rows 19-21: per iteration 4 blocks of 2 adds, one of 11, one of 22 -- not 8 groups)
  const double groups[NOPS] = {8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 4, 1, 1};
  const int adds[NOPS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 11, 22};
  // wave-instructions per SIMD: 8 waves/SIMD (256 CUs x 8 blocks x 4 waves / 1024 SIMDs) x iters x 8 chains
  printf("clock %d MHz (attribute); cycles per wavefront-instruction(-group) per SIMD at that clock:\n", clk_khz / 1000);
  for (int i = 0; i < NOPS; i++) {
    const double cyc = ms[i] * 1e-3 * clk_khz * 1e3 / (8.0 * iters * groups[i]);
    printf("  %-30s %8.3f ms   %6.2f cycles", names[i], ms[i], cyc);
    if (adds[i]) printf("   = %5.2f per add", cyc / adds[i]);
    printf("\n");
  }
  return 0;
}
