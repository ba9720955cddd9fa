// Binding-level attention functions (bindings.cpp): input checks, output
// allocation, the process-wide block order and the per-kernel timer.  The
// kernels and their launches are in attention_fwd.hip / attention_bwd.hip.
#include <string>
#include <vector>

#include "attention.h"

namespace lpp {

static int g_order_mode = [] {
  const char* e = getenv("LPP_ATTN_ORDER");
  return (e && e[0] == '0') ? 0 : 1;
}();

int attn_order_mode() { return g_order_mode; }

void attn_check_qkv(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                    const char* who) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16, who, ": bf16 only");
  TORCH_CHECK(q.dim() == 4 && q.size(3) == ATTN_D, who, ": [B,S,H,128] required");
  TORCH_CHECK(q.is_contiguous() && k.is_contiguous() && v.is_contiguous());
  TORCH_CHECK(q.size(2) % k.size(2) == 0);
}

void attn_check_docs(const at::Tensor& q, const at::Tensor& d, const char* who,
                     const char* name) {
  TORCH_CHECK(d.scalar_type() == at::kInt, who, ": ", name, " must be int32");
  TORCH_CHECK(d.is_contiguous(), who, ": ", name, " must be contiguous");
  TORCH_CHECK(d.dim() == 2 && d.size(0) == q.size(0) && d.size(1) == q.size(1), who, ": ",
              name, " must be [B,S]");
  TORCH_CHECK(d.device() == q.device(), who, ": ", name, " must be on q's device");
}

static void attn_check_bwd(const at::Tensor& dO, const at::Tensor& q, const at::Tensor& k,
                           const at::Tensor& v, const at::Tensor& o,
                           const at::Tensor& lse2, const char* who) {
  attn_check_qkv(q, k, v, who);
  TORCH_CHECK(dO.is_contiguous() && o.is_contiguous() && lse2.is_contiguous());
}

}  // namespace lpp

std::vector<at::Tensor> attention_fwd(at::Tensor q, at::Tensor k, at::Tensor v) {
  lpp::attn_check_qkv(q, k, v, "attention_fwd");
  const int B = q.size(0), S = q.size(1), H = q.size(2);
  auto o = at::empty_like(q);
  auto lse2 = at::empty({B, H, S}, q.options().dtype(at::kFloat));
  lpp::launch_attn_fwd(q, k, v, o, lse2,
                       lpp::attn_order_mode() ? lpp::ATTN_MODE1_FWD : 0, 0);
  return {o, lse2};
}

std::vector<at::Tensor> attention_bwd(at::Tensor dO, at::Tensor q, at::Tensor k,
                                      at::Tensor v, at::Tensor o, at::Tensor lse2) {
  lpp::attn_check_bwd(dO, q, k, v, o, lse2, "attention_bwd");
  const int B = q.size(0), S = q.size(1), H = q.size(2);
  auto delta = at::empty({B, H, S}, q.options().dtype(at::kFloat));
  lpp::launch_attn_bwd_delta(dO, o, delta);
  auto dq = at::empty_like(q);
  auto dk = at::empty_like(k);
  auto dv = at::empty_like(v);
  const int mode = lpp::attn_order_mode();
  lpp::launch_attn_bwd_dq(dO, q, k, v, lse2, delta, dq, mode ? lpp::ATTN_MODE1_DQ : 0, 0);
  lpp::launch_attn_bwd_dkdv(dO, q, k, v, lse2, delta, dk, dv,
                            mode ? lpp::ATTN_MODE1_DKDV : 0, 0);
  return {dq, dk, dv};
}

// Packed rows: query i of row b sees keys doc_start[b][i] .. i.  doc_start is
// non-decreasing with doc_start[b][i] <= i, doc_end[b][j] is one past the last
// token of key j's document (lpp_amd.ops.DocLayout validates and derives them;
// the kernels index with them unchecked).
std::vector<at::Tensor> attention_fwd_docs(at::Tensor q, at::Tensor k, at::Tensor v,
                                           at::Tensor doc_start) {
  lpp::attn_check_qkv(q, k, v, "attention_fwd_docs");
  lpp::attn_check_docs(q, doc_start, "attention_fwd_docs", "doc_start");
  const int B = q.size(0), S = q.size(1), H = q.size(2);
  auto o = at::empty_like(q);
  auto lse2 = at::empty({B, H, S}, q.options().dtype(at::kFloat));
  lpp::launch_attn_fwd(q, k, v, o, lse2,
                       lpp::attn_order_mode() ? lpp::ATTN_MODE1_FWD : 0, 0, &doc_start);
  return {o, lse2};
}

std::vector<at::Tensor> attention_bwd_docs(at::Tensor dO, at::Tensor q, at::Tensor k,
                                           at::Tensor v, at::Tensor o, at::Tensor lse2,
                                           at::Tensor doc_start, at::Tensor doc_end) {
  lpp::attn_check_bwd(dO, q, k, v, o, lse2, "attention_bwd_docs");
  lpp::attn_check_docs(q, doc_start, "attention_bwd_docs", "doc_start");
  lpp::attn_check_docs(q, doc_end, "attention_bwd_docs", "doc_end");
  const int B = q.size(0), S = q.size(1), H = q.size(2);
  auto delta = at::empty({B, H, S}, q.options().dtype(at::kFloat));
  lpp::launch_attn_bwd_delta(dO, o, delta);
  auto dq = at::empty_like(q);
  auto dk = at::empty_like(k);
  auto dv = at::empty_like(v);
  const int mode = lpp::attn_order_mode();
  lpp::launch_attn_bwd_dq(dO, q, k, v, lse2, delta, dq, mode ? lpp::ATTN_MODE1_DQ : 0, 0,
                          &doc_start);
  lpp::launch_attn_bwd_dkdv(dO, q, k, v, lse2, delta, dk, dv,
                            mode ? lpp::ATTN_MODE1_DKDV : 0, 0, &doc_end);
  return {dq, dk, dv};
}

void attention_set_block_order(int64_t mode) {
  TORCH_CHECK(mode == 0 || mode == 1, "attention_set_block_order: mode 0 or 1");
  lpp::g_order_mode = (int)mode;
}

int64_t attention_get_block_order() { return lpp::g_order_mode; }

// Host only: the (blk, head) pairs of L = 0..n-1 from the header function the
// kernels run.  kind 0 = fwd/dQ, 1 = dK/dV.
at::Tensor attention_block_order(int64_t kind, int64_t nblk, int64_t nheads, int64_t G,
                                 int64_t mode) {
  TORCH_CHECK(kind == 0 || kind == 1, "attention_block_order: kind 0 (fwd/dQ) or 1 (dK/dV)");
  TORCH_CHECK(mode == 0 || mode == 1, "attention_block_order: mode 0 or 1");
  TORCH_CHECK(nblk >= 1 && nheads >= 1 && nblk * nheads < (int64_t)1 << 30 && G >= 1);
  G = std::min(G, nheads);
  const int n = (int)(nblk * nheads);
  auto out = at::empty({n, 2}, at::TensorOptions().dtype(at::kInt));
  int* p = out.data_ptr<int>();
  for (int L = 0; L < n; ++L) {
    const lpp::AttnBlock ob =
        lpp::attn_block_order(L, (int)nblk, (int)nheads, (int)G, (int)kind, (int)mode);
    p[2 * L] = ob.blk;
    p[2 * L + 1] = ob.head;
  }
  return out;
}

// Host only: the 64 per-lane LDS byte addresses (within one image) of one access
// the kernels issue, from the header functions they run (attn_tile.h).  shape =
// 32 (32x32x16: forward, dQ) or 16 (16x16x32: dK/dV):
//   "stage"  ds_write_b128 of wave idx>>1, pass idx&1                (idx < 16)
//   "row"    ds_read_b128 A-fragment: shape 32 idx = t2*8 + dc       (idx < 16)
//                                     shape 16 idx = rt*4 + dc       (idx < 16)
//   "tr"     ds_read_b64_tr_b16, h = idx&1 of the two reads of a B-fragment:
//            shape 32 idx = (dt*4 + ks)*2 + h, shape 16 idx = (dt*2 + half)*2 + h
//                                                                    (idx < 32)
at::Tensor attention_lds_addresses(std::string pattern, int64_t shape, int64_t idx) {
  TORCH_CHECK(shape == 32 || shape == 16, "attention_lds_addresses: shape 32 or 16");
  const bool stage = pattern == "stage", row = pattern == "row", tr = pattern == "tr";
  TORCH_CHECK(stage || row || tr, "attention_lds_addresses: pattern is stage, row or tr");
  TORCH_CHECK(idx >= 0 && idx < (tr ? 32 : 16), "attention_lds_addresses: idx out of range");
  auto out = at::empty({64}, at::TensorOptions().dtype(at::kInt));
  int* p = out.data_ptr<int>();
  const int i = (int)idx;
  for (int lane = 0; lane < 64; ++lane) {
    if (stage)
      p[lane] = shape == 32 ? lpp::attn_stage_off<32>(i >> 1, i & 1, lane)
                            : lpp::attn_stage_off<16>(i >> 1, i & 1, lane);
    else if (row)
      p[lane] = shape == 32 ? lpp::attn_row_off32(lane, i >> 3, i & 7)
                            : lpp::attn_row_off16(lane, i >> 2, i & 3);
    else
      p[lane] = shape == 32 ? lpp::attn_tr_off32(lane, i >> 3, (i >> 1) & 3, i & 1)
                            : lpp::attn_tr_off16(lane, i >> 2, (i >> 1) & 1, i & 1);
  }
  return out;
}

// Device-timed A/B of one attention kernel under an explicit block order:
// kernel "fwd" | "dq" | "dkdv", order (mode, G; G <= 0 = the computed group).
// One hipEvent pair per launch; returns the ms of each of `reps` launches
// after `warmup` untimed ones.  With doc_start and doc_end (both or neither)
// the launches are those of the packed-row (_docs) functions.
std::vector<double> attention_time_kernel(std::string kernel, at::Tensor dO, at::Tensor q,
                                          at::Tensor k, at::Tensor v, at::Tensor o,
                                          at::Tensor lse2, int64_t mode, int64_t G,
                                          int64_t warmup, int64_t reps,
                                          c10::optional<at::Tensor> doc_start,
                                          c10::optional<at::Tensor> doc_end) {
  lpp::attn_check_bwd(dO, q, k, v, o, lse2, "attention_time_kernel");
  TORCH_CHECK(doc_start.has_value() == doc_end.has_value(),
              "attention_time_kernel: doc_start and doc_end come together");
  const at::Tensor* ds = nullptr;
  const at::Tensor* de = nullptr;
  if (doc_start.has_value()) {
    lpp::attn_check_docs(q, *doc_start, "attention_time_kernel", "doc_start");
    lpp::attn_check_docs(q, *doc_end, "attention_time_kernel", "doc_end");
    ds = &*doc_start;
    de = &*doc_end;
  }
  TORCH_CHECK(mode == 0 || mode == 1, "attention_time_kernel: mode 0 or 1");
  TORCH_CHECK(kernel == "fwd" || kernel == "dq" || kernel == "dkdv",
              "attention_time_kernel: kernel is fwd, dq or dkdv");
  const int B = q.size(0), S = q.size(1), H = q.size(2);
  auto delta = at::empty({B, H, S}, q.options().dtype(at::kFloat));
  lpp::launch_attn_bwd_delta(dO, o, delta);
  auto o2 = at::empty_like(q), dq = at::empty_like(q);
  auto lse_out = at::empty_like(lse2);
  auto dk = at::empty_like(k), dv = at::empty_like(v);
  auto launch = [&] {
    if (kernel == "fwd") lpp::launch_attn_fwd(q, k, v, o2, lse_out, (int)mode, (int)G, ds);
    else if (kernel == "dq")
      lpp::launch_attn_bwd_dq(dO, q, k, v, lse2, delta, dq, (int)mode, (int)G, ds);
    else lpp::launch_attn_bwd_dkdv(dO, q, k, v, lse2, delta, dk, dv, (int)mode, (int)G, de);
  };
  auto stream = lpp::current_stream();
  hipEvent_t e0, e1;
  LPP_CHECK_HIP(hipEventCreate(&e0));
  LPP_CHECK_HIP(hipEventCreate(&e1));
  for (int64_t i = 0; i < warmup; ++i) launch();
  std::vector<double> ms;
  for (int64_t i = 0; i < reps; ++i) {
    LPP_CHECK_HIP(hipEventRecord(e0, stream));
    launch();
    LPP_CHECK_HIP(hipEventRecord(e1, stream));
    LPP_CHECK_HIP(hipEventSynchronize(e1));
    float t = 0.f;
    LPP_CHECK_HIP(hipEventElapsedTime(&t, e0, e1));
    ms.push_back(t);
  }
  LPP_CHECK_HIP(hipEventDestroy(e0));
  LPP_CHECK_HIP(hipEventDestroy(e1));
  return ms;
}
