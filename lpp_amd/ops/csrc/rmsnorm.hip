// RMSNorm forward + backward for gfx950.
//
// Memory-bound: one workgroup (256 threads = 4 waves) per row, bf16 elements
// moved as 16-byte packets (8 x bf16). Forward reads x once, writes y + a
// per-row fp32 inv_rms for backward. Backward recomputes nothing: one pass
// for the per-row dot, one for dx, with dw accumulated per block and flushed
// to a [blocks, H] partial buffer that one torch sum reduces (no atomics).
//
// Reference op: HF LlamaRMSNorm as used by the reference repo
// (models/llama_ds_mp_wrap.py:12,184-188). Oracle: lpp_amd.ops.rmsnorm_ref.
#include "common.h"

namespace lpp {

constexpr int BLOCK = 256;

template <typename T, int VEC>
__global__ void rmsnorm_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                   T* __restrict__ y, float* __restrict__ invrms,
                                   int64_t n_rows, int H, float eps) {
  __shared__ float red[BLOCK / kWave];
  for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const T* xr = x + row * H;
    T* yr = y + row * H;
    using PV = Pack<T, VEC>;
    float ss = 0.f;
    for (int i = threadIdx.x * VEC; i < H; i += BLOCK * VEC) {
      PV buf = *reinterpret_cast<const PV*>(xr + i);
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        float f = to_f32(buf.v[v]);
        ss += f * f;
      }
    }
    float total = block_reduce_sum<BLOCK>(ss, red);
    float inv = rsqrtf(total / (float)H + eps);
    if (threadIdx.x == 0) invrms[row] = inv;
    for (int i = threadIdx.x * VEC; i < H; i += BLOCK * VEC) {
      PV xin = *reinterpret_cast<const PV*>(xr + i);
      PV out;
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        out.v[v] = from_f32<T>(to_f32(xin.v[v]) * inv * w[i + v]);
      *reinterpret_cast<PV*>(yr + i) = out;
    }
  }
}

// Scalar fallback for H not divisible by 16 bytes.
template <typename T>
__global__ void rmsnorm_fwd_kernel_s(const T* __restrict__ x, const float* __restrict__ w,
                                     T* __restrict__ y, float* __restrict__ invrms,
                                     int64_t n_rows, int H, float eps) {
  __shared__ float red[BLOCK / kWave];
  for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const T* xr = x + row * H;
    T* yr = y + row * H;
    float ss = 0.f;
    for (int i = threadIdx.x; i < H; i += BLOCK) {
      float f = to_f32(xr[i]);
      ss += f * f;
    }
    float total = block_reduce_sum<BLOCK>(ss, red);
    float inv = rsqrtf(total / (float)H + eps);
    if (threadIdx.x == 0) invrms[row] = inv;
    for (int i = threadIdx.x; i < H; i += BLOCK)
      yr[i] = from_f32<T>(to_f32(xr[i]) * inv * w[i]);
  }
}

// Gradient of the norm output at one element.  With NDY > 1 the partial
// gradients of sibling consumers (q/k/v, gate/up) are summed here in list
// order with a bf16 rounding after every add — the rounding the separate
// elementwise bf16 adds of the unfused path apply.
template <typename T, int NDY>
__device__ __forceinline__ T sum_partials(T a, T b, T c) {
  if (NDY >= 2) a = from_f32<T>(to_f32(a) + to_f32(b));
  if (NDY >= 3) a = from_f32<T>(to_f32(a) + to_f32(c));
  return a;
}

// Vectorised backward for H % VEC == 0 and H <= BLOCK*VEC*MAXIT (the
// production shapes): dy/x move as 16-byte packets, each packet is loaded
// ONCE and kept in registers for both the dot and the dx pass, and the
// per-thread dw partials accumulate in REGISTERS across the row loop
// (thread i's column set is row-invariant) and flush as one vectorised
// non-atomic store per block into dw_partial[block][H]; the host reduces
// partials with a single torch sum. Deterministic dw (no atomics).
// dx = inv*w*dy - x*inv^3/H * dot;  dw = sum_rows(dy*x*inv).
//
// Fused form (rmsnorm_bwd_fused): dy = sum of NDY partials (sum_partials),
// and with HAS_RES the residual-stream gradient is added to the rounded dx:
// dx_total = bf16(float(bf16(dx)) + float(dres)) — again the unfused path's
// rounding.  NDY = 1, HAS_RES = false is the plain backward.
template <typename T, int VEC, int N_IT, int NDY, bool HAS_RES>
__global__ __launch_bounds__(BLOCK) void rmsnorm_bwd_kernel_v(const T* __restrict__ dy, const T* __restrict__ dy1,
                                     const T* __restrict__ dy2, const T* __restrict__ dres,
                                     const T* __restrict__ x,
                                     const float* __restrict__ w,
                                     const float* __restrict__ invrms, T* __restrict__ dx,
                                     float* __restrict__ dw_partial, int64_t n_rows,
                                     int H) {
  __shared__ float red[BLOCK / kWave];
  using PV = Pack<T, VEC>;
  // N_IT is compile-time so the packet/partial arrays stay in registers
  // (a runtime bound would dynamic-index them into scratch).
  alignas(16) float dwacc[N_IT][VEC];
  // w is row-invariant but the block-reduce barrier stops the compiler
  // hoisting its loads out of the row loop — preload to registers once.
  alignas(16) float wreg[N_IT][VEC];
#pragma unroll
  for (int it = 0; it < N_IT; ++it) {
    const int i = threadIdx.x * VEC + it * BLOCK * VEC;
    *reinterpret_cast<Pack<float, 4>*>(&wreg[it][0]) =
        *reinterpret_cast<const Pack<float, 4>*>(w + i);
    *reinterpret_cast<Pack<float, 4>*>(&wreg[it][4]) =
        *reinterpret_cast<const Pack<float, 4>*>(w + i + 4);
#pragma unroll
    for (int v = 0; v < VEC; ++v) dwacc[it][v] = 0.f;
  }

  for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const T* dyr = dy + row * H;
    const T* xr = x + row * H;
    T* dxr = dx + row * H;
    const float inv = invrms[row];
    PV dybuf[N_IT], xbuf[N_IT];
    float dot = 0.f;
#pragma unroll
    for (int it = 0; it < N_IT; ++it) {
      const int i = threadIdx.x * VEC + it * BLOCK * VEC;
      dybuf[it] = *reinterpret_cast<const PV*>(dyr + i);
      if (NDY >= 2) {
        PV p1 = *reinterpret_cast<const PV*>(dy1 + row * H + i);
        PV p2 = p1;
        if (NDY >= 3) p2 = *reinterpret_cast<const PV*>(dy2 + row * H + i);
#pragma unroll
        for (int v = 0; v < VEC; ++v)
          dybuf[it].v[v] = sum_partials<T, NDY>(dybuf[it].v[v], p1.v[v], p2.v[v]);
      }
      xbuf[it] = *reinterpret_cast<const PV*>(xr + i);
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        dot += to_f32(dybuf[it].v[v]) * wreg[it][v] * to_f32(xbuf[it].v[v]);
    }
    const float total = block_reduce_sum<BLOCK>(dot, red);
    const float k = total * inv * inv * inv / (float)H;
#pragma unroll
    for (int it = 0; it < N_IT; ++it) {
      const int i = threadIdx.x * VEC + it * BLOCK * VEC;
      PV out;
      PV rp;
      if (HAS_RES) rp = *reinterpret_cast<const PV*>(dres + row * H + i);
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const float d = to_f32(dybuf[it].v[v]);
        const float xi = to_f32(xbuf[it].v[v]);
        out.v[v] = from_f32<T>(d * wreg[it][v] * inv - xi * k);
        if (HAS_RES) out.v[v] = from_f32<T>(to_f32(out.v[v]) + to_f32(rp.v[v]));
        dwacc[it][v] += d * xi * inv;
      }
      *reinterpret_cast<PV*>(dxr + i) = out;
    }
  }
  float* my = dw_partial + (int64_t)blockIdx.x * H;
#pragma unroll
  for (int it = 0; it < N_IT; ++it) {
    const int i = threadIdx.x * VEC + it * BLOCK * VEC;
    *reinterpret_cast<Pack<float, 4>*>(my + i) = *reinterpret_cast<Pack<float, 4>*>(&dwacc[it][0]);
    *reinterpret_cast<Pack<float, 4>*>(my + i + 4) = *reinterpret_cast<Pack<float, 4>*>(&dwacc[it][4]);
  }
}

// Any-shape fallback, same fused form.  dw accumulates per block in LDS and
// is flushed to dw_partial[block][H] like the vectorised kernel (no atomics,
// so dw is order-deterministic for every shape).
// dx = inv * w * dy - x * inv^3 / H * sum(dy * w * x)
// dw = sum_rows(dy * x * inv)
template <typename T, int NDY, bool HAS_RES>
__global__ void rmsnorm_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ dy1,
                                   const T* __restrict__ dy2, const T* __restrict__ dres,
                                   const T* __restrict__ x,
                                   const float* __restrict__ w,
                                   const float* __restrict__ invrms, T* __restrict__ dx,
                                   float* __restrict__ dw_partial, int64_t n_rows,
                                   int H) {
  __shared__ float red[BLOCK / kWave];
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* dw_loc = reinterpret_cast<float*>(smem);  // [H]
  for (int i = threadIdx.x; i < H; i += BLOCK) dw_loc[i] = 0.f;
  __syncthreads();

  for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const T* dyr = dy + row * H;
    const T* xr = x + row * H;
    T* dxr = dx + row * H;
    const float inv = invrms[row];
    float dot = 0.f;
    for (int i = threadIdx.x; i < H; i += BLOCK) {
      float d = to_f32(sum_partials<T, NDY>(dyr[i], NDY >= 2 ? dy1[row * H + i] : dyr[i],
                                            NDY >= 3 ? dy2[row * H + i] : dyr[i]));
      float xi = to_f32(xr[i]);
      dot += d * w[i] * xi;
      dw_loc[i] += d * xi * inv;
    }
    float total = block_reduce_sum<BLOCK>(dot, red);
    float k = total * inv * inv * inv / (float)H;
    for (int i = threadIdx.x; i < H; i += BLOCK) {
      float d = to_f32(sum_partials<T, NDY>(dyr[i], NDY >= 2 ? dy1[row * H + i] : dyr[i],
                                            NDY >= 3 ? dy2[row * H + i] : dyr[i]));
      float xi = to_f32(xr[i]);
      T o = from_f32<T>(d * w[i] * inv - xi * k);
      if (HAS_RES) o = from_f32<T>(to_f32(o) + to_f32(dres[row * H + i]));
      dxr[i] = o;
    }
  }
  __syncthreads();
  float* my = dw_partial + (int64_t)blockIdx.x * H;
  for (int i = threadIdx.x; i < H; i += BLOCK) my[i] = dw_loc[i];
}

}  // namespace lpp

std::vector<at::Tensor> rmsnorm_fwd(at::Tensor x, at::Tensor weight, double eps) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(), "rmsnorm_fwd: x must be contiguous on GPU");
  const int H = x.size(-1);
  const int64_t n_rows = x.numel() / H;
  auto y = at::empty_like(x);
  auto invrms = at::empty({n_rows}, x.options().dtype(at::kFloat));
  auto w32 = weight.to(at::kFloat).contiguous();
  auto stream = lpp::current_stream();
  const int grid = lpp::grid_for(n_rows, 1, 4096);
  LPP_DISPATCH_FLOAT(x.scalar_type(), "rmsnorm_fwd", [&] {
    constexpr int VEC = 16 / sizeof(scalar_t);
    if (H % VEC == 0) {
      hipLaunchKernelGGL((lpp::rmsnorm_fwd_kernel<scalar_t, VEC>), dim3(grid),
                         dim3(lpp::BLOCK), 0, stream, (const scalar_t*)x.data_ptr(),
                         w32.data_ptr<float>(), (scalar_t*)y.data_ptr(),
                         invrms.data_ptr<float>(), n_rows, H, (float)eps);
    } else {
      hipLaunchKernelGGL((lpp::rmsnorm_fwd_kernel_s<scalar_t>), dim3(grid),
                         dim3(lpp::BLOCK), 0, stream, (const scalar_t*)x.data_ptr(),
                         w32.data_ptr<float>(), (scalar_t*)y.data_ptr(),
                         invrms.data_ptr<float>(), n_rows, H, (float)eps);
    }
  });
  LPP_CHECK_HIP(hipGetLastError());
  return {y, invrms};
}

namespace lpp {

// Shared launcher of rmsnorm_bwd and rmsnorm_bwd_fused: dys holds 1..3
// partial gradients (summed in list order), dres is optional.
static std::vector<at::Tensor> rmsnorm_bwd_launch(const std::vector<at::Tensor>& dys,
                                                  at::Tensor x, at::Tensor weight,
                                                  at::Tensor invrms,
                                                  const c10::optional<at::Tensor>& dres) {
  const int H = x.size(-1);
  const int64_t n_rows = x.numel() / H;
  auto dx = at::empty_like(x);
  auto dw32 = at::empty({H}, x.options().dtype(at::kFloat));
  auto w32 = weight.to(at::kFloat).contiguous();
  auto stream = current_stream();
  const int ndy = (int)dys.size();
  const bool has_res = dres.has_value();
  LPP_DISPATCH_FLOAT(x.scalar_type(), "rmsnorm_bwd", [&] {
    constexpr int VEC = 16 / sizeof(scalar_t);
    const scalar_t* p0 = (const scalar_t*)dys[0].data_ptr();
    const scalar_t* p1 = ndy >= 2 ? (const scalar_t*)dys[1].data_ptr() : p0;
    const scalar_t* p2 = ndy >= 3 ? (const scalar_t*)dys[2].data_ptr() : p0;
    const scalar_t* pr = has_res ? (const scalar_t*)dres->data_ptr() : p0;
    const int n_it = H / (BLOCK * VEC);
    const bool vec = VEC == 8 && H % (BLOCK * VEC) == 0 && n_it >= 1 && n_it <= 4;
    const int grid = grid_for(n_rows, 1, vec ? 2048 : 1024);
    auto partial = at::empty({grid, H}, x.options().dtype(at::kFloat));
    const size_t lds = vec ? 0 : (size_t)H * sizeof(float);
    TORCH_CHECK(lds <= 160 * 1024 - 4096, "rmsnorm_bwd: H too large for LDS dw buffer");
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(grid), dim3(BLOCK), lds, stream, p0, p1, p2, pr,
                         (const scalar_t*)x.data_ptr(), w32.data_ptr<float>(),
                         invrms.data_ptr<float>(), (scalar_t*)dx.data_ptr(),
                         partial.data_ptr<float>(), n_rows, H);
    };
    // (ndy, has_res) -> compile-time kernel variant
    auto pick = [&](auto ndy_c, auto res_c) {
      constexpr int NDY = decltype(ndy_c)::value;
      constexpr bool RES = decltype(res_c)::value;
      if (!vec) launch(rmsnorm_bwd_kernel<scalar_t, NDY, RES>);
      else if (n_it == 1) launch(rmsnorm_bwd_kernel_v<scalar_t, VEC, 1, NDY, RES>);
      else if (n_it == 2) launch(rmsnorm_bwd_kernel_v<scalar_t, VEC, 2, NDY, RES>);
      else if (n_it == 3) launch(rmsnorm_bwd_kernel_v<scalar_t, VEC, 3, NDY, RES>);
      else launch(rmsnorm_bwd_kernel_v<scalar_t, VEC, 4, NDY, RES>);
    };
    auto pick_res = [&](auto ndy_c) {
      if (has_res) pick(ndy_c, std::true_type{});
      else pick(ndy_c, std::false_type{});
    };
    if (ndy == 1) pick_res(std::integral_constant<int, 1>{});
    else if (ndy == 2) pick_res(std::integral_constant<int, 2>{});
    else pick_res(std::integral_constant<int, 3>{});
    LPP_CHECK_HIP(hipGetLastError());
    at::sum_out(dw32, partial, {0});
  });
  return {dx, dw32.to(weight.scalar_type())};
}

}  // namespace lpp

std::vector<at::Tensor> rmsnorm_bwd(at::Tensor dy, at::Tensor x, at::Tensor weight,
                                    at::Tensor invrms) {
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() && x.is_contiguous());
  return lpp::rmsnorm_bwd_launch({dy}, x, weight, invrms, c10::nullopt);
}

at::Tensor transpose2d(at::Tensor in);

// Norm backward with the surrounding gradient adds fused in:
//   dy       = dys[0] (+ dys[1] (+ dys[2])), a bf16 rounding after each add
//   dx_total = bf16(rmsnorm_bwd(dy)) + dres, rounded once more
// i.e. exactly what separate elementwise adds around rmsnorm_bwd compute, in
// one pass.  Returns {dx_total, dw, dxT}; dxT is dx_total^T ([H, rows]) when
// want_t is set and the shape is tile-aligned bf16, else an empty tensor.
// The row-per-block kernel has no 64-row tile to transpose from (and its
// row -> block assignment fixes the bits of dw), so dxT is written by the
// transpose2d kernel straight after the norm kernel.
std::vector<at::Tensor> rmsnorm_bwd_fused(std::vector<at::Tensor> dys, at::Tensor x,
                                          at::Tensor weight, at::Tensor invrms,
                                          c10::optional<at::Tensor> dres, bool want_t) {
  TORCH_CHECK(!dys.empty() && dys.size() <= 3, "rmsnorm_bwd_fused: 1..3 partial gradients");
  TORCH_CHECK(x.is_cuda() && x.is_contiguous());
  auto check = [&](const at::Tensor& t, const char* what) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == x.scalar_type() &&
                    t.numel() == x.numel() && t.size(-1) == x.size(-1),
                "rmsnorm_bwd_fused: ", what, " must match x (contiguous, same dtype/shape)");
  };
  for (const auto& t : dys) check(t, "dys");
  if (dres.has_value()) check(*dres, "dres");
  auto out = lpp::rmsnorm_bwd_launch(dys, x, weight, invrms, dres);
  const int64_t H = x.size(-1), rows = x.numel() / H;
  if (want_t && x.scalar_type() == at::kBFloat16 && rows % 64 == 0 && H % 128 == 0)
    out.push_back(transpose2d(out[0].view({rows, H})));
  else
    out.push_back(at::empty({0}, x.options()));
  return out;
}
