// Fused cross-entropy over bf16 logits (fwd + bwd), gfx950.
//
// Semantics: per-row CE with ignore_index=-100, returning (sum of losses,
// per-row logsumexp, valid-row count). The Python wrapper does the causal
// shift and the mean (reference loss_fn, models/llama_ds_mp_wrap.py:105-116).
//
// Why fused: eager CE upcasts the [B*S, V] logits to fp32
// (4.3 GB per 65B microbatch at mbs 8) and materialises softmax; here logits
// stay bf16, forward saves only an [N] fp32 logsumexp, and backward emits
// dlogits = scale * (softmax - onehot) in a single pass.
//
// One 256-thread block per row; online (max, sumexp) in one read pass.
// Oracle: lpp_amd.ops.shifted_cross_entropy_ref.
#include "common.h"

namespace lpp {

constexpr int CE_BLOCK = 256;

template <typename T, int VEC>
__global__ void ce_fwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ labels,
                              float* __restrict__ loss_sum, float* __restrict__ lse_out,
                              int* __restrict__ count, int64_t n_rows, int V) {
  __shared__ float red[CE_BLOCK / kWave];
  using PV = Pack<T, VEC>;
  for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const T* lr = logits + row * V;
    // online per-thread (m, s)
    float m = -INFINITY, s = 0.f;
    const int nv = V / VEC;
    for (int i = threadIdx.x; i < nv; i += CE_BLOCK) {
      PV p = reinterpret_cast<const PV*>(lr)[i];
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        float x = to_f32(p.v[v]);
        if (x > m) {
          s *= __expf(m - x);
          m = x;
        }
        s += __expf(x - m);
      }
    }
    for (int i = nv * VEC + threadIdx.x; i < V; i += CE_BLOCK) {
      float x = to_f32(lr[i]);
      if (x > m) {
        s *= __expf(m - x);
        m = x;
      }
      s += __expf(x - m);
    }
    // block combine
    float gm = block_reduce_max<CE_BLOCK>(m, red);
    float gs = block_reduce_sum<CE_BLOCK>(s * __expf(m - gm), red);
    float lse = gm + __logf(gs);
    const int64_t lab = labels[row];
    if (threadIdx.x == 0) {
      lse_out[row] = lse;
      if (lab >= 0) {
        float gold = to_f32(lr[lab]);
        atomicAdd(loss_sum, lse - gold);
        atomicAdd(count, 1);
      }
    }
    __syncthreads();
  }
}

template <typename T, int VEC>
__global__ void ce_bwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ labels,
                              const float* __restrict__ lse, T* __restrict__ dlogits,
                              float scale, int64_t n_rows, int V) {
  using PV = Pack<T, VEC>;
  for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const T* lr = logits + row * V;
    T* dr = dlogits + row * V;
    const int64_t lab = labels[row];
    const float l = lse[row];
    const int nv = V / VEC;
    if (lab < 0) {
      // ignored row: zero grad
      PV z;
#pragma unroll
      for (int v = 0; v < VEC; ++v) z.v[v] = from_f32<T>(0.f);
      for (int i = threadIdx.x; i < nv; i += CE_BLOCK) reinterpret_cast<PV*>(dr)[i] = z;
      for (int i = nv * VEC + threadIdx.x; i < V; i += CE_BLOCK) dr[i] = from_f32<T>(0.f);
      continue;
    }
    for (int i = threadIdx.x; i < nv; i += CE_BLOCK) {
      PV p = reinterpret_cast<const PV*>(lr)[i];
      PV d;
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const int col = i * VEC + v;
        float sm = __expf(to_f32(p.v[v]) - l);
        d.v[v] = from_f32<T>(scale * (sm - (col == (int)lab ? 1.f : 0.f)));
      }
      reinterpret_cast<PV*>(dr)[i] = d;
    }
    for (int i = nv * VEC + threadIdx.x; i < V; i += CE_BLOCK) {
      float sm = __expf(to_f32(lr[i]) - l);
      dr[i] = from_f32<T>(scale * (sm - (i == (int)lab ? 1.f : 0.f)));
    }
  }
}

}  // namespace lpp

std::vector<at::Tensor> cross_entropy_fwd(at::Tensor logits, at::Tensor labels) {
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous() && logits.dim() == 2);
  TORCH_CHECK(labels.scalar_type() == at::kLong && labels.is_contiguous());
  const int64_t n_rows = logits.size(0);
  const int V = logits.size(1);
  TORCH_CHECK(labels.numel() == n_rows);
  auto loss_sum = at::zeros({}, logits.options().dtype(at::kFloat));
  auto lse = at::empty({n_rows}, logits.options().dtype(at::kFloat));
  auto count = at::zeros({}, logits.options().dtype(at::kInt));
  auto stream = lpp::current_stream();
  const int grid = lpp::grid_for(n_rows, 1, 2048);
  LPP_DISPATCH_FLOAT(logits.scalar_type(), "ce_fwd", [&] {
    constexpr int VEC = 16 / sizeof(scalar_t);
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(grid), dim3(lpp::CE_BLOCK), 0, stream,
                         (const scalar_t*)logits.data_ptr(), labels.data_ptr<int64_t>(),
                         loss_sum.data_ptr<float>(), lse.data_ptr<float>(),
                         count.data_ptr<int>(), n_rows, V);
    };
    // 16-byte packets need an aligned base and a row pitch that keeps every
    // row aligned; any other shape runs the one-element instantiation.
    if (V % VEC == 0 && lpp::aligned(logits.data_ptr(), 16))
      launch(lpp::ce_fwd_kernel<scalar_t, VEC>);
    else
      launch(lpp::ce_fwd_kernel<scalar_t, 1>);
  });
  LPP_CHECK_HIP(hipGetLastError());
  return {loss_sum, lse, count};
}

at::Tensor cross_entropy_bwd(at::Tensor logits, at::Tensor labels, at::Tensor lse,
                             double scale) {
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous() && logits.dim() == 2);
  const int64_t n_rows = logits.size(0);
  const int V = logits.size(1);
  TORCH_CHECK(labels.is_cuda() && labels.scalar_type() == at::kLong && labels.is_contiguous() &&
              labels.numel() == n_rows, "ce_bwd: labels must be [rows] int64 on GPU");
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == at::kFloat && lse.is_contiguous() &&
              lse.numel() == n_rows, "ce_bwd: lse must be [rows] fp32 on GPU");
  auto dlogits = at::empty_like(logits);
  auto stream = lpp::current_stream();
  const int grid = lpp::grid_for(n_rows, 1, 2048);
  LPP_DISPATCH_FLOAT(logits.scalar_type(), "ce_bwd", [&] {
    constexpr int VEC = 16 / sizeof(scalar_t);
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(grid), dim3(lpp::CE_BLOCK), 0, stream,
                         (const scalar_t*)logits.data_ptr(), labels.data_ptr<int64_t>(),
                         lse.data_ptr<float>(), (scalar_t*)dlogits.data_ptr(), (float)scale,
                         n_rows, V);
    };
    if (V % VEC == 0 && lpp::aligned(logits.data_ptr(), 16) &&
        lpp::aligned(dlogits.data_ptr(), 16))
      launch(lpp::ce_bwd_kernel<scalar_t, VEC>);
    else
      launch(lpp::ce_bwd_kernel<scalar_t, 1>);
  });
  LPP_CHECK_HIP(hipGetLastError());
  return dlogits;
}
