// What does the chip sustain on fp16 MFMAs alone, and does the MFMA shape matter under the power cap? One workgroup of 4 waves per
// CU (160 KiB of LDS requested so that exactly one is resident), each wave owns a 128x128 fp32 output tile (256 accumulator
// registers) and issues back-to-back MFMAs on it for ~40 ms per launch. Reports TFLOP/s from HIP events, the shader clock from
// s_memtime / s_memrealtime (100 MHz) and the board power from the amdgpu hwmon file.
//   default : the shape table. v_mfma_f32_32x32x16_f16 (4x4 blocks of 16 registers) against v_mfma_f32_16x16x32_f16 (8x8 blocks of
//             4), each from registers and with every fragment re-read from LDS by ds_read_b128 (16 reads per k = 32 in both shapes:
//             the same bytes). Random fp16 operands, 256 workgroups; every variant runs back to back for >= 2 s before its timed
//             launches, the variants interleaved over three rounds in this one process.
//   --sweep : 32x32x16 from registers, zero / random operands, 32..256 busy CUs (profiles/r04_mfma_power_limit.txt)
//   hipcc --offload-arch=gfx950 -O2 tools/micro/mfma_power_bench.hip -o tools/micro/mfma_power_bench && ./tools/micro/mfma_power_bench
#include <hip/hip_runtime.h>
#include <glob.h>
#include <unistd.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float16v __attribute__((ext_vector_type(16)));
typedef float float4v __attribute__((ext_vector_type(4)));

// Per wave and k = 32: 16 fragments of 16 bytes per lane (32x32x16: two k-steps of 4 X + 4 W fragments; 16x16x32: 8 X + 8 W).
// src holds two such sets per wave (k = 64 per loop iteration), staged at LDS [set][fragment][thread] (a lane's 16 bytes contiguous
// with its neighbours': conflict-free b128 reads). The loop is assembly (the compiler shuffles 64 four-register accumulators through
// copies): fragment sets in v[64:127] / v[128:191], accumulators a[0:255]; the register arm reads the sets once, the LDS arm reads
// each set again under the other set's MFMAs, one ds_read_b128 behind every 4th (16x16x32) / 2nd (32x32x16) MFMA.
#define D10(p) p "0", p "1", p "2", p "3", p "4", p "5", p "6", p "7", p "8", p "9"
#define D100(p) D10(p "0"), D10(p "1"), D10(p "2"), D10(p "3"), D10(p "4"), D10(p "5"), D10(p "6"), D10(p "7"), D10(p "8"), D10(p "9")
#define CLOBBERS "v64", "v65", "v66", "v67", "v68", "v69", D10("v7"), D10("v8"), D10("v9"), D10("v10"), D10("v11"), D10("v12"), D10("v13"), D10("v14"), \
  D10("v15"), D10("v16"), D10("v17"), D10("v18"), "v190", "v191", D10("a"), D10("a1"), D10("a2"), D10("a3"), D10("a4"), D10("a5"), D10("a6"), D10("a7"), D10("a8"), \
  D10("a9"), D100("a1"), D10("a20"), D10("a21"), D10("a22"), D10("a23"), D10("a24"), "a250", "a251", "a252", "a253", "a254", "a255", "memory", "scc"
// one set (k = 32) of MFMAs on the fragments from register `base`; READ: what follows each MFMA
#define SET16(base, READ) \
  ".irp rb,0,1,2,3,4,5,6,7\n.irp cb,0,1,2,3,4,5,6,7\n" \
  "v_mfma_f32_16x16x32_f16 a[(\\rb*8+\\cb)*4:(\\rb*8+\\cb)*4+3], v[" base "+32+\\cb*4:" base "+32+\\cb*4+3], v[" base "+\\rb*4:" base "+\\rb*4+3], a[(\\rb*8+\\cb)*4:(\\rb*8+\\cb)*4+3]\n" \
  READ ".endr\n.endr\n"
#define SET32(base, READ) \
  ".irp ks,0,1\n.irp rb,0,1,2,3\n.irp cb,0,1,2,3\n" \
  "v_mfma_f32_32x32x16_f16 a[(\\rb*4+\\cb)*16:(\\rb*4+\\cb)*16+15], v[" base "+\\ks*32+16+\\cb*4:" base "+\\ks*32+16+\\cb*4+3], v[" base "+\\ks*32+\\rb*4:" base "+\\ks*32+\\rb*4+3], a[(\\rb*4+\\cb)*16:(\\rb*4+\\cb)*16+15]\n" \
  READ ".endr\n.endr\n.endr\n"
#define READ16(other, addr) ".if ((\\rb*8+\\cb)&3)==3\nds_read_b128 v[" other "+((\\rb*8+\\cb)>>2)*4:" other "+((\\rb*8+\\cb)>>2)*4+3], " addr " offset:((\\rb*8+\\cb)>>2)*4096\n.endif\n"
#define READ32(other, addr) ".if ((\\ks*16+\\rb*4+\\cb)&1)==1\nds_read_b128 v[" other "+((\\ks*16+\\rb*4+\\cb)>>1)*4:" other "+((\\ks*16+\\rb*4+\\cb)>>1)*4+3], " addr " offset:((\\ks*16+\\rb*4+\\cb)>>1)*4096\n.endif\n"
#define LOOP(SET, R0, R1) \
  ".irp i,0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15\nds_read_b128 v[64+\\i*4:64+\\i*4+3], %4 offset:\\i*4096\nds_read_b128 v[128+\\i*4:128+\\i*4+3], %5 offset:\\i*4096\n.endr\n" \
  ".set psam_i, 0\n.rept 256\nv_accvgpr_write_b32 a[psam_i], 0\n.set psam_i, psam_i+1\n.endr\n" \
  "s_waitcnt lgkmcnt(0)\n" \
  "1:\n" SET("64", R1) "s_waitcnt lgkmcnt(0)\n" SET("128", R0) "s_waitcnt lgkmcnt(0)\n" \
  "s_sub_u32 %3, %3, 1\ns_cmp_lg_u32 %3, 0\ns_cbranch_scc1 1b\n" \
  "s_nop 7\ns_nop 7\ns_nop 7\ns_memtime %0\ns_memrealtime %1\ns_waitcnt lgkmcnt(0)\nv_accvgpr_read_b32 %2, a0\n"

template <bool M16, bool LDS> __global__ __launch_bounds__(256, 1) void shape_loop(const half8* __restrict__ src, float* __restrict__ sink, unsigned long long* __restrict__ stamps, int iters) {
  extern __shared__ half8 lds8[];
  const int tid = threadIdx.x;
  for (int i = 0; i < 32; ++i) lds8[i * 256 + tid] = src[(blockIdx.x * 32 + i) * 256 + tid];
  __syncthreads();
  unsigned long long c0, r0, c1, r1; float a0; int it = iters;
  const unsigned addr0 = tid * 16, addr1 = addr0 + 65536;
  // (the first stamps are taken before the 32 staging reads and the zeroing of the accumulators: ~1k cycles of 123 M)
  asm volatile("s_memtime %0\ns_memrealtime %1\ns_waitcnt lgkmcnt(0)\n" : "=s"(c0), "=s"(r0));
  if (M16 && LDS) asm volatile(LOOP(SET16, READ16("64", "%4"), READ16("128", "%5")) : "=&s"(c1), "=&s"(r1), "=v"(a0), "+s"(it) : "v"(addr0), "v"(addr1) : CLOBBERS);
  else if (M16) asm volatile(LOOP(SET16, "", "") : "=&s"(c1), "=&s"(r1), "=v"(a0), "+s"(it) : "v"(addr0), "v"(addr1) : CLOBBERS);
  else if (LDS) asm volatile(LOOP(SET32, READ32("64", "%4"), READ32("128", "%5")) : "=&s"(c1), "=&s"(r1), "=v"(a0), "+s"(it) : "v"(addr0), "v"(addr1) : CLOBBERS);
  else asm volatile(LOOP(SET32, "", "") : "=&s"(c1), "=&s"(r1), "=v"(a0), "+s"(it) : "v"(addr0), "v"(addr1) : CLOBBERS);
  if (a0 == 123.456f) sink[0] = a0;
  if (tid == 0) { stamps[blockIdx.x * 2] = c1 - c0; stamps[blockIdx.x * 2 + 1] = r1 - r0; }
}

__global__ __launch_bounds__(256, 1) void mfma_loop(const half8* __restrict__ src, float* __restrict__ sink, unsigned long long* __restrict__ stamps, int iters) {
  extern __shared__ char lds[];
  const int lane = threadIdx.x;
  half8 a[4], b[4];
  for (int i = 0; i < 4; ++i) { a[i] = src[(blockIdx.x * 8 + i) * 256 + lane]; b[i] = src[(blockIdx.x * 8 + 4 + i) * 256 + lane]; }
  float16v acc[8];
  for (int i = 0; i < 8; ++i) for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;
  unsigned long long c0 = __builtin_readcyclecounter(), r0 = wall_clock64();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[(i + u) & 3], b[i & 3], acc[i], 0, 0, 0);
    }
  }
  unsigned long long c1 = __builtin_readcyclecounter(), r1 = wall_clock64();
  float s = 0.f;
  for (int i = 0; i < 8; ++i) for (int j = 0; j < 16; ++j) s += acc[i][j];
  if (s == 123.456f) sink[0] = s;
  if (lane == 0) { stamps[blockIdx.x * 2] = c1 - c0; stamps[blockIdx.x * 2 + 1] = r1 - r0; }
  if (iters < 0) lds[lane] = 1;
}

// board power in W from the hwmon directory of the device with this PCI address (or of the only card); < 0: not readable
static std::string g_power_file;
static void find_power_file() {
  char bdf[64] = {0};
  hipDeviceGetPCIBusId(bdf, sizeof bdf, 0);
  for (char* p = bdf; *p; ++p) *p = (char)tolower(*p);
  glob_t g;
  if (glob("/sys/class/drm/card*/device/hwmon/hwmon*/power1_input", 0, nullptr, &g)) return;
  for (size_t i = 0; i < g.gl_pathc; ++i) {
    std::string dev = std::string(g.gl_pathv[i]);
    dev = dev.substr(0, dev.find("/hwmon/"));
    char real[4096];
    if (realpath(dev.c_str(), real) && strstr(real, bdf)) g_power_file = g.gl_pathv[i];
  }
  if (g_power_file.empty() && g.gl_pathc == 1) g_power_file = g.gl_pathv[0];
  globfree(&g);
}
static double read_power() {
  if (g_power_file.empty()) return -1.0;
  FILE* f = fopen(g_power_file.c_str(), "r");
  if (!f) return -1.0;
  double uw = -1e6;
  if (fscanf(f, "%lf", &uw) != 1) uw = -1e6;
  fclose(f);
  return uw * 1e-6;
}

static int sweep(half8* d, float* sink, unsigned long long* st, std::vector<_Float16>& h) {
  const int maxwg = 256;
  hipFuncSetAttribute((const void*)mfma_loop, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  for (int data = 0; data < 2; ++data) {
    srand(1);
    for (auto& v : h) v = data ? (_Float16)((rand() / (float)RAND_MAX) * 2.f - 1.f) : (_Float16)0.f;
    hipMemcpy(d, h.data(), (size_t)maxwg * 8 * 256 * 16, hipMemcpyHostToDevice);
    for (int wgs : {32, 64, 128, 192, 256}) {
      const int iters = 120000;   // x 32 MFMAs of 32 cycles = 123 M cycles per wave
      for (int rep = 0; rep < 2; ++rep) {
        hipEventRecord(e0);
        hipLaunchKernelGGL(mfma_loop, dim3(wgs), dim3(256), 160 * 1024, 0, d, sink, st, iters);
        hipEventRecord(e1); hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1);
        std::vector<unsigned long long> s(wgs * 2);
        hipMemcpy(s.data(), st, wgs * 16, hipMemcpyDeviceToHost);
        double cyc = 0, rt = 0;
        for (int i = 0; i < wgs; ++i) { cyc += s[2 * i]; rt += s[2 * i + 1]; }
        const double flop = (double)wgs * 4 * iters * 32.0 * 2 * 32 * 32 * 16;
        if (rep) printf("%s operands, %3d workgroups (4 waves, one per SIMD): %7.1f ms  %7.1f TFLOP/s  shader clock %5.0f MHz  %.2f cycles per MFMA\n", data ? "random" : "zero  ", wgs,
                        ms, flop / ms / 1e9, cyc / rt * 100.0, cyc / wgs / (iters * 32.0));
      }
    }
  }
  return 0;
}

typedef void (*kern_t)(const half8*, float*, unsigned long long*, int);

int main(int argc, char** argv) {
  const int wgs = 256;
  std::vector<_Float16> h((size_t)wgs * 32 * 256 * 8);
  half8* d; float* sink; unsigned long long* st;
  hipMalloc(&d, h.size() * 2); hipMalloc(&sink, 4); hipMalloc(&st, wgs * 16);
  if (argc > 1 && !strcmp(argv[1], "--sweep")) return sweep(d, sink, st, h);
  find_power_file();
  srand(1);
  for (auto& v : h) v = (_Float16)((rand() / (float)RAND_MAX) * 2.f - 1.f);
  hipMemcpy(d, h.data(), h.size() * 2, hipMemcpyHostToDevice);
  struct { const char* name; kern_t fn; } var[4] = {
    {"32x32x16 registers", shape_loop<false, false>}, {"16x16x32 registers", shape_loop<true, false>},
    {"32x32x16 LDS reads", shape_loop<false, true>}, {"16x16x32 LDS reads", shape_loop<true, true>}};
  for (auto& v : var) hipFuncSetAttribute((const void*)v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  const int iters = 30000;           // x 4096 MFMA cycles (k = 64 of a 128x128 tile) = 123 M cycles per wave and launch
  const double flop_launch = (double)wgs * 4 * iters * 2.0 * 128 * 128 * 64;
  printf("# %d workgroups of 4 waves (one per SIMD), 128x128 tile per wave, random fp16 operands; >= 2 s of launches before each timed window of 8\n", wgs);
  printf("# %-20s %5s %9s %10s %12s %11s %8s\n", "variant", "round", "ms/launch", "TFLOP/s", "cycles/kFLOP", "clock MHz", "power W");
  for (int round = 0; round < 3; ++round) {
    for (auto& v : var) {
      hipEventRecord(e0);
      float warm = 0.f;
      while (warm < 2000.f) {
        for (int i = 0; i < 8; ++i) hipLaunchKernelGGL(v.fn, dim3(wgs), dim3(256), 160 * 1024, 0, d, sink, st, iters);
        hipEventRecord(e1); hipEventSynchronize(e1);
        hipEventElapsedTime(&warm, e0, e1);
      }
      const int timed = 8;
      hipEventRecord(e0);
      for (int i = 0; i < timed; ++i) hipLaunchKernelGGL(v.fn, dim3(wgs), dim3(256), 160 * 1024, 0, d, sink, st, iters);
      hipEventRecord(e1);
      double psum = 0; int pn = 0;
      while (hipEventQuery(e1) == hipErrorNotReady) { double p = read_power(); if (p > 0) { psum += p; ++pn; } usleep(20000); }
      if (hipEventSynchronize(e1) != hipSuccess) { printf("launch failed: %s\n", hipGetErrorString(hipGetLastError())); return 1; }
      float ms; hipEventElapsedTime(&ms, e0, e1); ms /= timed;
      std::vector<unsigned long long> s(wgs * 2);
      hipMemcpy(s.data(), st, wgs * 16, hipMemcpyDeviceToHost);
      double cyc = 0, rt = 0;
      for (int i = 0; i < wgs; ++i) { cyc += s[2 * i]; rt += s[2 * i + 1]; }
      // cycles per 1000 FLOP of one SIMD: the wave's loop cycles over its share of the launch's FLOP
      printf("  %-20s %5d %9.2f %10.1f %12.4f %11.0f %8.0f\n", v.name, round, ms, flop_launch / ms / 1e9, (cyc / wgs) / (flop_launch / (wgs * 4)) * 1e3, cyc / rt * 100.0,
             pn ? psum / pn : -1.0);
      fflush(stdout);
    }
  }
  return 0;
}
