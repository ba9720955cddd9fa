// Fused SwiGLU: y = silu(gate) * up, forward + backward, gfx950.
//
// Pure elementwise / memory-bound: grid-stride, 16-byte packets per lane
// (8 x bf16). Backward recomputes sigmoid from the saved gate/up inputs —
// no intermediate is ever materialised (the eager path writes silu(g) to
// HBM and reads it back; SURVEY.md §2.7 MLP row).
//
// Oracle: lpp_amd.ops.swiglu_ref.
#include "common.h"
#include "transpose_tile.h"

namespace lpp {

template <typename T, int VEC>
__global__ void swiglu_fwd_kernel(const T* __restrict__ g, const T* __restrict__ u,
                                  T* __restrict__ y, int64_t n_vec) {
  using PV = Pack<T, VEC>;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_vec;
       i += (int64_t)gridDim.x * blockDim.x) {
    PV gp = reinterpret_cast<const PV*>(g)[i];
    PV up = reinterpret_cast<const PV*>(u)[i];
    PV yp;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      float gf = to_f32(gp.v[v]);
      float s = 1.f / (1.f + __expf(-gf));
      yp.v[v] = from_f32<T>(gf * s * to_f32(up.v[v]));
    }
    reinterpret_cast<PV*>(y)[i] = yp;
  }
}

template <typename T, int VEC>
__global__ void swiglu_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ g,
                                  const T* __restrict__ u, T* __restrict__ dg,
                                  T* __restrict__ du, int64_t n_vec) {
  using PV = Pack<T, VEC>;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_vec;
       i += (int64_t)gridDim.x * blockDim.x) {
    PV dyp = reinterpret_cast<const PV*>(dy)[i];
    PV gp = reinterpret_cast<const PV*>(g)[i];
    PV up = reinterpret_cast<const PV*>(u)[i];
    PV dgp, dup;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      float d = to_f32(dyp.v[v]);
      float gf = to_f32(gp.v[v]);
      float uf = to_f32(up.v[v]);
      float s = 1.f / (1.f + __expf(-gf));
      float silu = gf * s;
      float dsilu = s * (1.f + gf * (1.f - s));
      dgp.v[v] = from_f32<T>(d * uf * dsilu);
      dup.v[v] = from_f32<T>(d * silu);
    }
    reinterpret_cast<PV*>(dg)[i] = dgp;
    reinterpret_cast<PV*>(du)[i] = dup;
  }
}

// Tiled backward that also writes dg^T and du^T ([I, T]) for the wgrad GEMMs
// of gate_proj / up_proj: one workgroup per 64-row x 128-column tile, the
// arithmetic of swiglu_bwd_kernel line for line, natural b128 stores as
// before, plus one LDS image per output stored transposed (transpose_tile.h).
// Requires T % 64 == 0 and I % 128 == 0.
__global__ __launch_bounds__(256) void swiglu_bwd_t_kernel(
    const __hip_bfloat16* __restrict__ dy, const __hip_bfloat16* __restrict__ g,
    const __hip_bfloat16* __restrict__ u, __hip_bfloat16* __restrict__ dg,
    __hip_bfloat16* __restrict__ du, short* __restrict__ dgT, short* __restrict__ duT,
    int T, int I) {
  __shared__ __attribute__((aligned(16))) char img[2][kTTImgBytes];  // 32 KB
  using T_ = __hip_bfloat16;
  using PV = Pack<T_, 8>;

  const int r0 = blockIdx.y * 64;
  const int c0 = blockIdx.x * 128;

#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int64_t off = (int64_t)(r0 + tt_row(pass)) * I + c0 + tt_col();
    PV dyp = *reinterpret_cast<const PV*>(dy + off);
    PV gp = *reinterpret_cast<const PV*>(g + off);
    PV up = *reinterpret_cast<const PV*>(u + off);
    PV dgp, dup;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      float d = to_f32(dyp.v[v]);
      float gf = to_f32(gp.v[v]);
      float uf = to_f32(up.v[v]);
      float s = 1.f / (1.f + __expf(-gf));
      float silu = gf * s;
      float dsilu = s * (1.f + gf * (1.f - s));
      dgp.v[v] = from_f32<T_>(d * uf * dsilu);
      dup.v[v] = from_f32<T_>(d * silu);
    }
    *reinterpret_cast<PV*>(dg + off) = dgp;
    *reinterpret_cast<PV*>(du + off) = dup;
    tt_stage(img[0], *reinterpret_cast<const bf16x8_t*>(&dgp), pass);
    tt_stage(img[1], *reinterpret_cast<const bf16x8_t*>(&dup), pass);
  }
  __syncthreads();
  tt_store(img[0], dgT, T, r0, c0);
  tt_store(img[1], duT, T, r0, c0);
}

}  // namespace lpp

at::Tensor swiglu_fwd(at::Tensor gate, at::Tensor up) {
  TORCH_CHECK(gate.is_cuda() && gate.is_contiguous() && up.is_contiguous());
  TORCH_CHECK(gate.sizes() == up.sizes() && gate.scalar_type() == up.scalar_type());
  auto y = at::empty_like(gate);
  const int64_t n = gate.numel();
  auto stream = lpp::current_stream();
  LPP_DISPATCH_FLOAT(gate.scalar_type(), "swiglu_fwd", [&] {
    constexpr int VEC = 16 / sizeof(scalar_t);
    TORCH_CHECK(n % VEC == 0, "swiglu: numel must be divisible by ", VEC);
    const int64_t n_vec = n / VEC;
    const int grid = lpp::grid_for(n_vec, 256);
    hipLaunchKernelGGL((lpp::swiglu_fwd_kernel<scalar_t, VEC>), dim3(grid), dim3(256), 0,
                       stream, (const scalar_t*)gate.data_ptr(),
                       (const scalar_t*)up.data_ptr(), (scalar_t*)y.data_ptr(), n_vec);
  });
  LPP_CHECK_HIP(hipGetLastError());
  return y;
}

std::vector<at::Tensor> swiglu_bwd(at::Tensor dy, at::Tensor gate, at::Tensor up) {
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous());
  auto dg = at::empty_like(gate);
  auto du = at::empty_like(up);
  const int64_t n = gate.numel();
  auto stream = lpp::current_stream();
  LPP_DISPATCH_FLOAT(gate.scalar_type(), "swiglu_bwd", [&] {
    constexpr int VEC = 16 / sizeof(scalar_t);
    const int64_t n_vec = n / VEC;
    const int grid = lpp::grid_for(n_vec, 256);
    hipLaunchKernelGGL((lpp::swiglu_bwd_kernel<scalar_t, VEC>), dim3(grid), dim3(256), 0,
                       stream, (const scalar_t*)dy.data_ptr(),
                       (const scalar_t*)gate.data_ptr(), (const scalar_t*)up.data_ptr(),
                       (scalar_t*)dg.data_ptr(), (scalar_t*)du.data_ptr(), n_vec);
  });
  LPP_CHECK_HIP(hipGetLastError());
  return {dg, du};
}

// swiglu_bwd that also returns dg^T, du^T ([I, T]) when the flattened shape
// is tile-aligned bf16: {dg, du, dgT, duT}.  Any other shape runs the
// grid-stride kernel and returns {dg, du}.
std::vector<at::Tensor> swiglu_bwd_t(at::Tensor dy, at::Tensor gate, at::Tensor up) {
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() && gate.is_contiguous() &&
              up.is_contiguous());
  TORCH_CHECK(dy.sizes() == gate.sizes() && gate.sizes() == up.sizes() &&
              dy.scalar_type() == gate.scalar_type() &&
              gate.scalar_type() == up.scalar_type());
  const int64_t I = gate.dim() >= 1 ? gate.size(-1) : 0;
  const int64_t T = I > 0 ? gate.numel() / I : 0;
  if (gate.scalar_type() != at::kBFloat16 || T == 0 || T % 64 != 0 || I % 128 != 0 ||
      T / 64 > 65535 || T > INT32_MAX || I > INT32_MAX)
    return swiglu_bwd(dy, gate, up);
  auto dg = at::empty_like(gate);
  auto du = at::empty_like(up);
  auto dgT = at::empty({I, T}, gate.options());
  auto duT = at::empty({I, T}, gate.options());
  dim3 grid((unsigned)(I / 128), (unsigned)(T / 64));
  hipLaunchKernelGGL(lpp::swiglu_bwd_t_kernel, grid, dim3(256), 0, lpp::current_stream(),
                     (const __hip_bfloat16*)dy.data_ptr(),
                     (const __hip_bfloat16*)gate.data_ptr(),
                     (const __hip_bfloat16*)up.data_ptr(), (__hip_bfloat16*)dg.data_ptr(),
                     (__hip_bfloat16*)du.data_ptr(), (short*)dgT.data_ptr(),
                     (short*)duT.data_ptr(), (int)T, (int)I);
  LPP_CHECK_HIP(hipGetLastError());
  return {dg, du, dgT, duT};
}
