// Does v_mul_f64 with a SUBNORMAL multiplicand issue at the normal rate (gfx950)?  The exact TOED stage can feed a pixel
// byte to fp64 as the subnormal {low word = byte, high word = 0} = byte * 2^-1074 against taps scaled by 2^1000 and 2^74
//  instead of converting it; that only pays if the multiply does not slow down.
// One kernel, one instruction stream; the operand VALUES are arguments, so the two variants differ in nothing else:
//   normal:    m = (double)byte,   ck,          rk
//   subnormal: m = byte * 2^-1074, ck * 2^1000, rk * 2^74      (byte = lane-dependent, 0..255)
// KIND 0: 16 x  t_i = m * ck                          (every multiply has the subnormal operand)
// KIND 1:  8 x (t_i = m * ck ; t_i = t_i * rk ; acc_i += t_i)   (the tap of exact_mag / exact9)
// Variants alternate, REPS times each, in one launch sequence; 8 and 4 waves per SIMD like bank_conflict / issue_mix.
// Build: hipcc -O3 --offload-arch=gfx950 -o subnormal_mul subnormal_mul.hip ; run on the GPU box.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>

#define ITER 2048
#define REPS 6
// t_i = v[10 + 4 i : 11 + 4 i], acc_i = v[12 + 4 i : 13 + 4 i] (i = 0..7); m = v[42:43], ck = v[44:45], rk = v[46:47]
#define MUL1(D, S) "v_mul_f64 v[" #D "], v[" #S "], v[44:45]\n\t"
#define MUL2(D) "v_mul_f64 v[" #D "], v[" #D "], v[46:47]\n\t"
#define ADD3(A, D) "v_add_f64 v[" #A "], v[" #A "], v[" #D "]\n\t"
#define CLOB                                                                                                         \
    "v10", "v11", "v12", "v13", "v14", "v15", "v16", "v17", "v18", "v19", "v20", "v21", "v22", "v23", "v24", "v25", "v26", \
        "v27", "v28", "v29", "v30", "v31", "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42",    \
        "v43", "v44", "v45", "v46", "v47"

template <int KIND>
__global__ __launch_bounds__(256) void k(double *out, int sub, double ck, double rk)
{
    const unsigned byte = threadIdx.x & 255u;
    const double m = sub ? __builtin_bit_cast(double, (unsigned long long)byte) : (double)byte;
    asm volatile("v_mov_b32 v42, %0\n\tv_mov_b32 v43, %1\n\tv_mov_b32 v44, %2\n\tv_mov_b32 v45, %3\n\t"
                 "v_mov_b32 v46, %4\n\tv_mov_b32 v47, %5\n\t"
                 "v_mov_b32 v12, 0\n\tv_mov_b32 v13, 0\n\tv_mov_b32 v16, 0\n\tv_mov_b32 v17, 0\n\t"
                 "v_mov_b32 v20, 0\n\tv_mov_b32 v21, 0\n\tv_mov_b32 v24, 0\n\tv_mov_b32 v25, 0\n\t"
                 "v_mov_b32 v28, 0\n\tv_mov_b32 v29, 0\n\tv_mov_b32 v32, 0\n\tv_mov_b32 v33, 0\n\t"
                 "v_mov_b32 v36, 0\n\tv_mov_b32 v37, 0\n\tv_mov_b32 v40, 0\n\tv_mov_b32 v41, 0\n\t"
                 :
                 : "v"(__double2loint(m)), "v"(__double2hiint(m)), "v"(__double2loint(ck)), "v"(__double2hiint(ck)),
                   "v"(__double2loint(rk)), "v"(__double2hiint(rk))
                 : CLOB);
    for (int it = 0; it < ITER; ++it)
    {
        if (KIND == 0)
            asm volatile(MUL1(10:11, 42:43) MUL1(12:13, 42:43) MUL1(14:15, 42:43) MUL1(16:17, 42:43) MUL1(18:19, 42:43)
                         MUL1(20:21, 42:43) MUL1(22:23, 42:43) MUL1(24:25, 42:43) MUL1(26:27, 42:43) MUL1(28:29, 42:43)
                         MUL1(30:31, 42:43) MUL1(32:33, 42:43) MUL1(34:35, 42:43) MUL1(36:37, 42:43) MUL1(38:39, 42:43)
                         MUL1(40:41, 42:43) ::: CLOB);
        if (KIND == 1)
            asm volatile(MUL1(10:11, 42:43) MUL1(14:15, 42:43) MUL1(18:19, 42:43) MUL1(22:23, 42:43) MUL1(26:27, 42:43)
                         MUL1(30:31, 42:43) MUL1(34:35, 42:43) MUL1(38:39, 42:43)
                         MUL2(10:11) MUL2(14:15) MUL2(18:19) MUL2(22:23) MUL2(26:27) MUL2(30:31) MUL2(34:35) MUL2(38:39)
                         ADD3(12:13, 10:11) ADD3(16:17, 14:15) ADD3(20:21, 18:19) ADD3(24:25, 22:23) ADD3(28:29, 26:27)
                         ADD3(32:33, 30:31) ADD3(36:37, 34:35) ADD3(40:41, 38:39) ::: CLOB);
    }
    int lo, hi;
    asm volatile("v_mov_b32 %0, v12\n\tv_mov_b32 %1, v13" : "=v"(lo), "=v"(hi)::CLOB);
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = __hiloint2double(hi, lo);
}

#define MAX_W 8
static double h_out[256 * MAX_W * 256];

template <int KIND>
static void run(const char *name, double *d, int W)
{
    const int blocks = 256 * W, threads = 256, per_step = KIND == 0 ? 16 : 24;
    const double ck = 0.31830988618379067, rk = -0.7071067811865476; // any two normal taps
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    double cyc[2][REPS], first[2] = {0.0, 0.0};
    hipLaunchKernelGGL((k<KIND>), dim3(blocks), dim3(threads), 0, 0, d, 0, ck, rk); // warm-up
    (void)hipDeviceSynchronize();
    for (int rep = 0; rep < REPS; ++rep)
        for (int sub = 0; sub < 2; ++sub)
        {
            (void)hipEventRecord(e0);
            hipLaunchKernelGGL((k<KIND>), dim3(blocks), dim3(threads), 0, 0, d, sub, sub ? std::ldexp(ck, 1000) : ck,
                               sub ? std::ldexp(rk, 74) : rk);
            (void)hipEventRecord(e1);
            (void)hipEventSynchronize(e1);
            float ms = 0;
            (void)hipEventElapsedTime(&ms, e0, e1);
            cyc[sub][rep] = 2.4e9 * (ms * 1e-3) / ((double)W * ITER * per_step);
            if (rep == 0)
            {
                (void)hipMemcpy(h_out, d, sizeof(double) * 256, hipMemcpyDeviceToHost);
                first[sub] = h_out[255];
            }
        }
    for (int sub = 0; sub < 2; ++sub)
    {
        printf("%-34s %d waves/SIMD  %-9s", name, W, sub ? "subnormal" : "normal");
        for (int rep = 0; rep < REPS; ++rep)
            printf(" %6.3f", cyc[sub][rep]);
        printf("   min %.3f max %.3f cycles (at 2.4 GHz) per wave instruction\n", *std::min_element(cyc[sub], cyc[sub] + REPS),
               *std::max_element(cyc[sub], cyc[sub] + REPS));
    }
    if (KIND == 1) // the accumulated sums of lane 255 must be the same bits either way
        printf("%-34s acc(lane 255): normal %a  subnormal %a  %s\n", "", first[0], first[1],
               first[0] == first[1] ? "equal" : "DIFFERENT");
}

int main()
{
    double *d;
    (void)hipMalloc(&d, sizeof(double) * 256 * MAX_W * 256);
    for (int W : {8, 4})
    {
        run<0>("v_mul_f64 t, m, ck", d, W);
        run<1>("mul t,m,ck; mul t,t,rk; add a,a,t", d, W);
    }
    return 0;
}
