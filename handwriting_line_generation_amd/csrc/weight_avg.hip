// Weight averaging (SWA / EMA, base/base_trainer.py:233-237, 481-484 of the reference) over the trainers' flat parameter table: the running
// mean of every parameter lives in ONE fp32 buffer laid out like FlatParams.flat_grad (tensor k at float offsets[k], segments padded to 16
// bytes), and two multi-tensor kernels walk the chunk table Adam walks:
//   weight_average : avg = avg * (1 - alpha) + p * alpha, with the reference's two roundings per element (no FMA)
//   weight_exchange: p <-> avg in place (validate / sample with the averaged weights, then put the live ones back)
// Both are pure streaming: 16-byte accesses over the aligned body of a piece, scalar accesses on the tail. The padding floats between the
// segments of avg are never read or written.
#include "hwg_common.h"

namespace {

constexpr int WA_U = 4;         // 16-byte pieces per stream in flight per thread
constexpr int WA_SPLIT = 16;    // workgroups per chunk-table entry (gridDim.y); an entry shorter than WA_MIN * WA_SPLIT elements uses fewer of them
constexpr int WA_MIN = 4096;    // fewest elements a workgroup takes (a multiple of 4: every piece starts 16-byte aligned when the tensor does)

struct WaArgs {
  const long long* ptrs;        // [nt] parameter addresses
  const int* chunk_tensor;      // [nchunks]
  const long long* chunk_off;   // [nchunks] first element of the entry within its tensor
  const long long* numel;       // [nt]
  const long long* offsets;     // [nt] first float of tensor t in avg
  int nchunks;
  float* avg;
};

// element range [off, end) of tensor t this workgroup owns. An entry of the chunk table ends where the tensor's next entry begins (entries
// of one tensor are consecutive and ascending) or at the tensor's end; it is cut into gridDim.y pieces whose length is a multiple of 4.
__device__ __forceinline__ bool wa_range(const WaArgs& a, int& t, long long& off, long long& end) {
  const int c = blockIdx.x;
  t = a.chunk_tensor[c];
  const long long o = a.chunk_off[c];
  long long e = a.numel[t];
  if (c + 1 < a.nchunks && a.chunk_tensor[c + 1] == t) e = min(e, a.chunk_off[c + 1]);
  long long sub = ((e - o + gridDim.y - 1) / gridDim.y + 3) & ~3LL;
  if (sub < WA_MIN) sub = WA_MIN;
  off = o + (long long)blockIdx.y * sub;
  end = min(e, off + sub);
  return off < end;
}

// fadd_rn(fmul_rn(a, oma), fmul_rn(p, alpha)): two products and one sum, each rounded to nearest. Written with plain operators under
// `fp contract(off)` and NOT with __fmul_rn / __fadd_rn: in this ROCm those are inline functions over `x * y` / `x + y` compiled under the
// header's own contraction state (hipcc's default -ffp-contract=fast-honor-pragmas), and the compiler fused them into v_pk_fma_f32 - one
// rounding instead of two - even with the pragma around the calls. The pragma governs the operators of THIS function: v_mul, v_mul, v_add.
__device__ __forceinline__ float wa_mix(float a, float p, float oma, float alpha) {
#pragma clang fp contract(off)
  const float x = a * oma;
  const float y = p * alpha;
  return x + y;
}

__global__ __launch_bounds__(256) void weight_average_kernel(WaArgs a, float oma, float alpha) {
  int t;
  long long off, end;
  if (!wa_range(a, t, off, end)) return;
  const float* p = reinterpret_cast<const float*>(a.ptrs[t]);
  if (!p) return;
  float* avg = a.avg + a.offsets[t];
  const bool al = ((reinterpret_cast<uintptr_t>(p + off) | reinterpret_cast<uintptr_t>(avg + off)) & 15) == 0;
  const long long n4 = al ? (end - off) >> 2 : 0;
  const float4* p4 = reinterpret_cast<const float4*>(p + off);
  float4* a4 = reinterpret_cast<float4*>(avg + off);
  for (long long j0 = threadIdx.x; j0 < n4; j0 += WA_U * 256) {
    float4 pv[WA_U], av[WA_U];
#pragma unroll
    for (int u = 0; u < WA_U; ++u) {
      const long long ju = j0 + u * 256 < n4 ? j0 + u * 256 : j0;
      pv[u] = p4[ju];
      av[u] = a4[ju];
    }
#pragma unroll
    for (int u = 0; u < WA_U; ++u) {
      const long long j = j0 + u * 256;
      if (j < n4)
        a4[j] = make_float4(wa_mix(av[u].x, pv[u].x, oma, alpha), wa_mix(av[u].y, pv[u].y, oma, alpha), wa_mix(av[u].z, pv[u].z, oma, alpha),
                            wa_mix(av[u].w, pv[u].w, oma, alpha));
    }
  }
  for (long long i = off + 4 * n4 + threadIdx.x; i < end; i += 256) avg[i] = wa_mix(avg[i], p[i], oma, alpha);
}

__global__ __launch_bounds__(256) void weight_exchange_kernel(WaArgs a) {
  int t;
  long long off, end;
  if (!wa_range(a, t, off, end)) return;
  float* p = reinterpret_cast<float*>(a.ptrs[t]);
  if (!p) return;
  float* avg = a.avg + a.offsets[t];
  const bool al = ((reinterpret_cast<uintptr_t>(p + off) | reinterpret_cast<uintptr_t>(avg + off)) & 15) == 0;
  const long long n4 = al ? (end - off) >> 2 : 0;
  // (the parameters and avg are separate allocations: __restrict__ lets the loads of the unrolled trips be issued ahead of the stores)
  float4* __restrict__ p4 = reinterpret_cast<float4*>(p + off);
  float4* __restrict__ a4 = reinterpret_cast<float4*>(avg + off);
#pragma unroll WA_U
  for (long long j = threadIdx.x; j < n4; j += 256) {
    const float4 pv = p4[j], av = a4[j];
    p4[j] = av;
    a4[j] = pv;
  }
  for (long long i = off + 4 * n4 + threadIdx.x; i < end; i += 256) {
    const float pv = p[i], av = avg[i];
    p[i] = av;
    avg[i] = pv;
  }
}

WaArgs make_wa(const void* param_ptrs, const void* chunk_tensor, const void* chunk_off, const void* numel, const void* offsets, int nchunks, float* avg) {
  WaArgs a;
  a.ptrs = (const long long*)param_ptrs; a.chunk_tensor = (const int*)chunk_tensor; a.chunk_off = (const long long*)chunk_off;
  a.numel = (const long long*)numel; a.offsets = (const long long*)offsets; a.nchunks = nchunks; a.avg = avg;
  return a;
}

}  // namespace

extern "C" int hwg_weight_average(const void* param_ptrs, const void* chunk_tensor, const void* chunk_off, const void* numel, const void* offsets,
                                  int nchunks, float* avg, float one_minus_alpha, float alpha, void* stream) {
  HWG_REQUIRE(param_ptrs && chunk_tensor && chunk_off && numel && offsets && avg && nchunks > 0, "weight_average: bad arguments");
  const WaArgs a = make_wa(param_ptrs, chunk_tensor, chunk_off, numel, offsets, nchunks, avg);
  hipLaunchKernelGGL(weight_average_kernel, dim3(nchunks, WA_SPLIT), dim3(256), 0, (hipStream_t)stream, a, one_minus_alpha, alpha);
  HWG_LAUNCH_CHECK("weight_average");
  return HWG_OK;
}

extern "C" int hwg_weight_exchange(const void* param_ptrs, const void* chunk_tensor, const void* chunk_off, const void* numel, const void* offsets,
                                   int nchunks, float* avg, void* stream) {
  HWG_REQUIRE(param_ptrs && chunk_tensor && chunk_off && numel && offsets && avg && nchunks > 0, "weight_exchange: bad arguments");
  const WaArgs a = make_wa(param_ptrs, chunk_tensor, chunk_off, numel, offsets, nchunks, avg);
  hipLaunchKernelGGL(weight_exchange_kernel, dim3(nchunks, WA_SPLIT), dim3(256), 0, (hipStream_t)stream, a);
  HWG_LAUNCH_CHECK("weight_exchange");
  return HWG_OK;
}
