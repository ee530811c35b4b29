// checkpoint.hip — vg_checkpoint_save / vg_checkpoint_load: a context's state
// that outlives a scan (the arrays lifetime.hip's compaction remaps, the
// estimator's DState, the host mirror) to one file and back.
//
// Save: complete the outstanding work, compact (lifetime.hip: afterwards the
// live map is a dense prefix of the node pool and of the point_fix arena),
// collect the root hash's (key, id) pairs ordered by id, then one launch packs
// every live prefix into a contiguous device image (k_ckpt_copy over a
// descriptor list, 16-byte accesses), two launches checksum every section
// (k_ckpt_sum / k_ckpt_sum2), one copy brings the image to pinned memory, and
// the file is written. The file's size follows the live map, never the slab.
// Load: read, validate header and table (ckpt_file.cpp), upload the image,
// recompute the checksums with the same kernels, check the capacities, parse
// the host mirror's blob — and only then touch the context: vg_reset, the
// inverse scatter (the same copy kernel, descriptors reversed), the root hash
// rebuilt by lifetime.hip's bidding rounds, DState's semantic fields one by
// one (never the struct: its publication numbers belong to the loading
// context), the host mirror.
#include <hipcub/hipcub.hpp>
#include <cstdio>
#include "ckpt_file.h"
#include "vg_dev.h"
#include "vg_reduce.h"

namespace vg {
namespace {

struct CopyDesc {
  const void* src;
  void* dst;
  unsigned long long bytes;  // a multiple of 4
};
constexpr int kCopyX = 64;    // workgroups per descriptor (grid-stride inside)
constexpr int kSumX = 128;    // partial sums per section

// One descriptor per blockIdx.y: bytes from src to dst with the widest access
// both addresses allow (16 bytes wherever the arrays' own alignment holds: the
// slab carves at 256 bytes, the image's sections start at 16), the sub-vector
// tail in 32-bit words.
__global__ void __launch_bounds__(256) k_ckpt_copy(const CopyDesc* __restrict__ desc) {
  const CopyDesc d = desc[blockIdx.y];
  const uintptr_t a = (uintptr_t)d.src | (uintptr_t)d.dst;
  const int v = (a & 15) == 0 ? 16 : (a & 7) == 0 ? 8 : 4;
  const unsigned long long nv = d.bytes / v;
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  const unsigned long long t0 = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (v == 16) {
    const uint4* s = (const uint4*)d.src;
    uint4* o = (uint4*)d.dst;
    for (unsigned long long i = t0; i < nv; i += stride) o[i] = s[i];
  } else if (v == 8) {
    const uint2* s = (const uint2*)d.src;
    uint2* o = (uint2*)d.dst;
    for (unsigned long long i = t0; i < nv; i += stride) o[i] = s[i];
  } else {
    const uint32_t* s = (const uint32_t*)d.src;
    uint32_t* o = (uint32_t*)d.dst;
    for (unsigned long long i = t0; i < nv; i += stride) o[i] = s[i];
  }
  const unsigned long long done = nv * v, tail = (d.bytes - done) / 4;  // < 4 words
  if (blockIdx.x == 0 && threadIdx.x < tail)
    ((uint32_t*)((char*)d.dst + done))[threadIdx.x] = ((const uint32_t*)((const char*)d.src + done))[threadIdx.x];
}

struct SumDesc {
  unsigned long long off, words;  // in the image; 64-bit words (the last one zero-padded in the image)
};
// Section blockIdx.y, partial blockIdx.x: sum of word[i] * (kCkptMul * (2 i + 1))
// over this workgroup's share, two words per 16-byte load; 64-lane shuffles,
// one partial per workgroup (no atomics, no last-workgroup ticket)
__global__ void __launch_bounds__(256) k_ckpt_sum(const unsigned char* __restrict__ img, const SumDesc* __restrict__ sec,
                                                  unsigned long long* __restrict__ part) {
  const SumDesc d = sec[blockIdx.y];
  const ulonglong2* w2 = (const ulonglong2*)(img + d.off);
  const unsigned long long pairs = d.words / 2;
  unsigned long long acc = 0;
  for (unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; j < pairs;
       j += (unsigned long long)gridDim.x * blockDim.x) {
    const ulonglong2 w = w2[j];
    acc += w.x * (kCkptMul * (4 * j + 1)) + w.y * (kCkptMul * (4 * j + 3));
  }
  if ((d.words & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned long long i = d.words - 1;
    acc += ((const unsigned long long*)(img + d.off))[i] * (kCkptMul * (2 * i + 1));
  }
  __shared__ unsigned long long sh[4];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}
__global__ void __launch_bounds__(kSumX) k_ckpt_sum2(const unsigned long long* __restrict__ part,
                                                     unsigned long long* __restrict__ out) {
  __shared__ unsigned long long sh[kSumX / 64];
  const unsigned long long acc = wave_sum(part[(size_t)blockIdx.x * kSumX + threadIdx.x]);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int k = 0; k < kSumX / 64; k++) t += sh[k];
    out[blockIdx.x] = t;
  }
}

// The root hash's (id, key) pairs, appended a wave at a time: one atomic per
// wave reserves the run, each lane takes its rank in the ballot. Append order
// is not kept: the pairs are sorted by id afterwards.
__global__ void __launch_bounds__(256) k_ckpt_roots(DevMap m, int n, int cap, int* __restrict__ cnt, int* __restrict__ ids,
                                                    uint64_t* __restrict__ keys) {
  const int hs = m.hash_mask + 1;
  const int lane = threadIdx.x & 63;
  const int rounds = (hs + gridDim.x * blockDim.x - 1) / (gridDim.x * blockDim.x);
  for (int t = 0; t < rounds; t++) {  // (every lane of a wave runs every round: the ballot below is wave-wide)
    const int s = (t * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
    uint64_t key = kKeyEmpty;
    int r = -1;
    if (s < hs) {
      key = m.hkey[s];
      r = m.hval[s];
    }
    const bool valid = key != kKeyEmpty && r >= 0 && r < n;
    const unsigned long long mask = __ballot(valid);
    if (!mask) continue;
    const int leader = __ffsll((long long)mask) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(cnt, __popcll(mask));
    base = __shfl(base, leader, 64);
    const int q = base + __popcll(mask & ((1ull << lane) - 1));
    if (valid && q < cap) {
      ids[q] = r;
      keys[q] = key;
    }
  }
}
// load: the pairs filed by id for the bidding rounds (lifetime.hip map_hash_place)
__global__ void __launch_bounds__(256) k_ckpt_hash_seed(int hash_mask, int n, int nroots, const int* __restrict__ ids,
                                                        const uint64_t* __restrict__ keys, uint64_t* __restrict__ rkey,
                                                        int* __restrict__ pos, int* __restrict__ bad) {
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < nroots; q += gridDim.x * blockDim.x) {
    const int id = ids[q];
    if (id < 0 || id >= n || (q > 0 && ids[q - 1] >= id)) {  // ordered by id, each once
      atomicOr(bad, 1);
      continue;
    }
    rkey[id] = keys[q];
    pos[id] = (int)hash_slot(keys[q], hash_mask);
  }
}

// The leaf runs (wp_ord, located by lseg) in canonical form. Where a run sits
// in its slot's wp_ord is decided by atomics (insert.hip k_ins_resolve's
// segment order, recut.hip's arena cursor) and no result depends on it; the
// file orders each slot's runs by node id — the insert's from entry 0, the
// recut's from cap_wp — so it is a function of the map alone. Stale lseg words
// (an older slot epoch) become 0. Cell (2 slot + region) n + node of cnt holds
// the run's length; its exclusive scan is the run's place in the section.
__device__ __forceinline__ bool run_of(const DevMap& m, int n, long e, int* slot, int* node, uint64_t* v) {
  *slot = (int)(e / n);
  *node = (int)(e - (long)*slot * n);
  *v = m.lseg[(size_t)*node * m.W + *slot];
  int st, len;
  return lseg_get(m, *node, *slot, st, len);  // a run of the slot's current epoch
}
__global__ void __launch_bounds__(256) k_ckpt_runs_count(DevMap m, int n, int* __restrict__ cnt) {
  const long total = (long)m.W * n;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int slot, node;
    uint64_t v;
    const bool ok = run_of(m, n, e, &slot, &node, &v);
    const int len = ok ? (int)((v >> 24) & 0x1fffff) : 0;
    const int region = (int)(v & 0xffffff) >= m.cap_wp ? 1 : 0;
    cnt[(size_t)(2 * slot) * n + node] = region == 0 ? len : 0;
    cnt[(size_t)(2 * slot + 1) * n + node] = region == 1 ? len : 0;
  }
}
__global__ void __launch_bounds__(256) k_ckpt_runs_pack(DevMap m, int n, const int* __restrict__ off, long ord_cap,
                                                        int* __restrict__ ord_img, uint64_t* __restrict__ lseg_img) {
  const long total = (long)m.W * n;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int slot, node;
    uint64_t v;
    uint64_t out = 0;
    if (run_of(m, n, e, &slot, &node, &v)) {
      const int st = (int)(v & 0xffffff), len = (int)((v >> 24) & 0x1fffff);
      const int region = st >= m.cap_wp ? 1 : 0;
      const size_t cell = (size_t)(2 * slot + region) * n;
      const long g = off[cell + node];                  // in the section
      const int rel = (int)(g - off[cell]);             // in the slot's region
      if (st + len <= m.ord_stride && g + len <= ord_cap) {
        const int* src = m.wp_ord + (size_t)slot * m.ord_stride + st;
        for (int j = 0; j < len; j++) ord_img[g + j] = src[j];
        out = lseg_pack(region ? m.cap_wp + rel : rel, len, (int)(v >> 45));
      }
    }
    lseg_img[(size_t)node * m.W + slot] = out;
  }
}

struct PinBuf {  // a pinned host allocation freed at scope exit
  void* p = nullptr;
  ~PinBuf() {
    if (p) (void)hipHostFree(p);
  }
};
using Scratch = DevBuf<char>;  // device scratch of one call, in bytes
#define CK_ALLOC(buf, bytes, what)                                                                         \
  do {                                                                                                     \
    const hipError_t e_ = (buf).reserve((bytes) > 0 ? (size_t)(bytes) : 64);                               \
    if (e_ != hipSuccess) {                                                                                \
      ctx->err = std::string(who) + ": " + what + " (" + std::to_string((size_t)(bytes) >> 20) + " MiB): " + \
                 hipGetErrorString(e_);                                                                    \
      return VG_E_HIP;                                                                                     \
    }                                                                                                      \
  } while (0)

// The image's layout, from the dimensions alone: the section table (offsets,
// byte counts) and the copy list between the context's arrays and the image.
// The same function serves both directions (to_image false: src and dst swap).
struct Layout {
  std::vector<CkptSec> sec;
  std::vector<CopyDesc> copy;
  uint64_t image_bytes = 0;
};
void add_section(Layout& L, uint32_t id, int W, uint64_t count) {
  CkptSec s;
  memset(&s, 0, sizeof(s));
  s.id = id;
  s.rec = ckpt_rec(id, W);
  s.count = count;
  s.bytes = count * s.rec;
  s.off = L.image_bytes;
  L.image_bytes = (s.off + s.bytes + 15) & ~uint64_t(15);
  L.sec.push_back(s);
}
void build_layout(vg_ctx* ctx, const CkptDims& d, uint64_t host_bytes, char* img, bool to_image, Layout& L) {
  const DevMap& m = ctx->map;
  const int W = d.W;
  auto piece = [&](const void* arr, uint64_t img_off, uint64_t bytes) {
    if (bytes == 0) return;
    bytes = (bytes + 3) & ~uint64_t(3);
    CopyDesc c;
    c.src = to_image ? arr : (const void*)(img + img_off);
    c.dst = to_image ? (void*)(img + img_off) : const_cast<void*>(arr);
    c.bytes = bytes;
    L.copy.push_back(c);
  };
  auto whole = [&](uint32_t id, const void* arr, uint64_t count) {
    add_section(L, id, W, count);
    piece(arr, L.sec.back().off, L.sec.back().bytes);
  };
  const uint64_t n = (uint64_t)d.n_nodes;
  whole(kSecHdr, m.hdr, n);
  whole(kSecPlane, m.pl, n);
  whole(kSecPcrAdd, m.pcr_add, n);
  whole(kSecPcrFix, m.pcr_fix, n);
  whole(kSecCovAdd, m.cov_add, n);
  whole(kSecEig, m.eig, n);
  whole(kSecJour, m.jour, n);
  whole(kSecDbox, m.dbox, n);
  whole(kSecPcrs, m.pcrs, n);
  // lseg and wp_ord: on save written in canonical form by k_ckpt_runs_pack (below), on load copied as they are
  add_section(L, kSecLseg, W, n);
  if (!to_image) piece(m.lseg, L.sec.back().off, L.sec.back().bytes);
  whole(kSecInSlide, m.in_slide, n);  // (copied in 32-bit words: the bytes past n are the zeroed tail's)
  whole(kSecSlide, m.slide, (uint64_t)d.n_slide);
  whole(kSecFixPnt, m.fix_pnt, (uint64_t)d.n_fix);
  whole(kSecFixVar, m.fix_var, (uint64_t)d.n_fix);
  // the window points: every physical slot's first wpn points, slot after slot
  uint64_t wp = 0, ord = 0;
  for (int s = 0; s < 32; s++) {
    wp += (uint64_t)d.wpn[s];
    ord += (uint64_t)d.ord0[s] + (uint64_t)(d.arena[s] > d.cap_wp ? d.arena[s] - d.cap_wp : 0);
  }
  struct WpArr {
    uint32_t id;
    const char* base;
  };
  const WpArr wps[] = {{kSecWpPnt, (const char*)m.wp_pnt}, {kSecWpVar, (const char*)m.wp_var},
                       {kSecWpLeaf, (const char*)m.wp_leaf}, {kSecWpInt, (const char*)m.wp_int}};
  for (const WpArr& a : wps) {
    add_section(L, a.id, W, wp);
    const uint64_t rec = L.sec.back().rec;
    uint64_t at = L.sec.back().off;
    for (int s = 0; s < W; s++) {
      piece(a.base + (uint64_t)s * m.cap_wp * rec, at, (uint64_t)d.wpn[s] * rec);
      at += (uint64_t)d.wpn[s] * rec;
    }
  }
  // wp_ord per slot: the insert's runs [0, ord0), then the recut's arena [cap_wp, cursor)
  add_section(L, kSecWpOrd, W, ord);
  if (!to_image) {
    uint64_t at = L.sec.back().off;
    for (int s = 0; s < W; s++) {
      const int* base = m.wp_ord + (size_t)s * m.ord_stride;
      piece(base, at, (uint64_t)d.ord0[s] * 4);
      at += (uint64_t)d.ord0[s] * 4;
      const uint64_t extra = d.arena[s] > d.cap_wp ? (uint64_t)(d.arena[s] - d.cap_wp) : 0;
      piece(base + d.cap_wp, at, extra * 4);
      at += extra * 4;
    }
  }
  // slot_epoch[32] and the map counters (wpn and the arena cursors travel in the header's dimensions)
  add_section(L, kSecSlots, W, kCkptSlotInts);
  piece(m.slot_epoch, L.sec.back().off, 32 * 4);
  piece(m.counters, L.sec.back().off + 32 * 4, (uint64_t)kCntN * 4);
  // the root pairs: written by the sort on save, read by k_ckpt_hash_seed on load (no copy)
  add_section(L, kSecRootId, W, (uint64_t)d.n_roots);
  add_section(L, kSecRootKey, W, (uint64_t)d.n_roots);
  // DState, the semantic fields in a fixed order
  add_section(L, kSecDState, W, kCkptDStateDoubles);
  {
    uint64_t at = L.sec.back().off;
    const DState* st = ctx->st;
    auto field = [&](const void* p, uint64_t bytes) {
      piece(p, at, bytes);
      at += bytes;
    };
    field(st->xc, sizeof(st->xc));
    field(st->xp, sizeof(st->xp));
    field(st->G6, sizeof(st->G6));
    field(st->nnt, sizeof(st->nnt));
    field(st->traj, sizeof(st->traj));
    field(st->xs, sizeof(st->xs));
    field(st->bias, sizeof(st->bias));
    field(&st->jour, sizeof(double));
    field(st->last_pos, sizeof(st->last_pos));
    field(st->imurec, sizeof(st->imurec));
    field(&st->imu_head, sizeof(int));  // (the other half of the word stays zero)
  }
  add_section(L, kSecHost, W, host_bytes);  // host memory: copied by the caller
}

int run_copy(vg_ctx* ctx, const Layout& L, const char* who) {
  if (L.copy.empty()) return VG_OK;
  Scratch dd;
  CK_ALLOC(dd, L.copy.size() * sizeof(CopyDesc), "descriptor list");
  VG_HIP(hipMemcpyAsync(dd.p, L.copy.data(), L.copy.size() * sizeof(CopyDesc), hipMemcpyHostToDevice, ctx->stream));
  k_ckpt_copy<<<dim3(kCopyX, (unsigned)L.copy.size()), kBlock, 0, ctx->stream>>>((const CopyDesc*)dd.p);
  VG_HIP(hipGetLastError());
  VG_HIP(hipStreamSynchronize(ctx->stream));  // (the descriptor list is freed on return)
  return VG_OK;
}

// every section's checksum, on the device, into sums[nsec]
int run_sums(vg_ctx* ctx, const unsigned char* img, const std::vector<CkptSec>& sec, uint64_t* sums, const char* who) {
  const size_t ns = sec.size();
  std::vector<SumDesc> sd(ns);
  for (size_t i = 0; i < ns; i++) {
    sd[i].off = sec[i].off;
    sd[i].words = (sec[i].bytes + 7) / 8;
  }
  Scratch b;
  const size_t o_part = (ns * sizeof(SumDesc) + 255) & ~size_t(255), o_out = o_part + ns * kSumX * 8;
  CK_ALLOC(b, o_out + ns * 8, "checksum scratch");
  char* p = (char*)b.p;
  VG_HIP(hipMemcpyAsync(p, sd.data(), ns * sizeof(SumDesc), hipMemcpyHostToDevice, ctx->stream));
  k_ckpt_sum<<<dim3(kSumX, (unsigned)ns), kBlock, 0, ctx->stream>>>(img, (const SumDesc*)p, (unsigned long long*)(p + o_part));
  k_ckpt_sum2<<<(unsigned)ns, kSumX, 0, ctx->stream>>>((const unsigned long long*)(p + o_part),
                                                        (unsigned long long*)(p + o_out));
  VG_HIP(hipGetLastError());
  VG_HIP(hipMemcpyAsync(sums, p + o_out, ns * 8, hipMemcpyDeviceToHost, ctx->stream));
  VG_HIP(hipStreamSynchronize(ctx->stream));
  return VG_OK;
}

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
}  // namespace

// t_ms (may be null; scripts/probe_checkpoint.py): [0] compaction + root collection, [1] pack + checksum,
// [2] device -> pinned host, [3] file write
int checkpoint_save(vg_ctx* ctx, const char* path, long long* bytes, double* t_ms) {
  const char* who = "vg_checkpoint_save";
  VG_TRY(host_ckpt_allowed(ctx, who, true));
  VG_TRY(host_sync(ctx));
  hipStream_t s = ctx->stream;
  DevMap& m = ctx->map;
  double t0 = now_ms();
  long long rel[6];
  VG_TRY(map_release(ctx, false, 0, 0.0, 1, rel));  // the compaction (no release): the live map becomes a dense prefix
  // dimensions
  CkptDims d;
  memset(&d, 0, sizeof(d));
  int hc[kCntN];
  VG_HIP(hipMemcpyAsync(hc, m.counters, sizeof(hc), hipMemcpyDeviceToHost, s));
  VG_HIP(hipMemcpyAsync(d.wpn, m.wpn, sizeof(d.wpn), hipMemcpyDeviceToHost, s));
  VG_HIP(hipMemcpyAsync(d.arena, m.arena, sizeof(d.arena), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  if (hc[kCntErr]) {
    ctx->err = std::string(who) + ": the map holds an error (flags " + std::to_string(hc[kCntErr]) + ")";
    return VG_E_STATE;
  }
  d.n_nodes = hc[kCntNodes];
  d.n_fix = hc[kCntFix];
  d.n_slide = hc[kCntSlide];
  d.W = m.W;
  d.cap_wp = m.cap_wp;
  d.max_layer = ctx->cfg.max_layer;
  for (int k = d.W; k < 32; k++) d.wpn[k] = d.arena[k] = 0;
  // the root pairs, appended in any order, then ordered by id
  const size_t un = (size_t)(d.n_nodes > 0 ? d.n_nodes : 1);
  Scratch rb;
  const size_t o_ids = 256, o_keys = (o_ids + un * 4 + 255) & ~size_t(255), o_end = o_keys + un * 8;
  CK_ALLOC(rb, o_end, "root scratch");
  char* rp = (char*)rb.p;
  VG_HIP(hipMemsetAsync(rp, 0, 256, s));
  k_ckpt_roots<<<grid_for((long)m.hash_mask + 1), kBlock, 0, s>>>(m, d.n_nodes, (int)un, (int*)rp, (int*)(rp + o_ids),
                                                                  (uint64_t*)(rp + o_keys));
  VG_HIP(hipGetLastError());
  VG_HIP(hipMemcpyAsync(&d.n_roots, rp, sizeof(int), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  if (d.n_roots > d.n_nodes) {
    ctx->err = std::string(who) + ": more hashed roots than nodes";
    return VG_E_STATE;
  }
  // the leaf runs' canonical places (k_ckpt_runs_count): one scan over (slot, region, node)
  const size_t cells = (size_t)2 * d.W * un + 1;
  Scratch runs;
  size_t scan_tb = 0;
  VG_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_tb, (int*)nullptr, (int*)nullptr, (int)cells, s));
  const size_t o_off = (cells * 4 + 255) & ~size_t(255), o_tmp = o_off + ((cells * 4 + 255) & ~size_t(255));
  CK_ALLOC(runs, o_tmp + scan_tb, "leaf run scratch");
  int* run_cnt = (int*)runs.p;
  int* run_off = (int*)((char*)runs.p + o_off);
  VG_HIP(hipMemsetAsync(run_cnt, 0, cells * 4, s));
  if (d.n_nodes > 0) k_ckpt_runs_count<<<grid_for((long)d.W * d.n_nodes), kBlock, 0, s>>>(m, d.n_nodes, run_cnt);
  VG_HIP(hipGetLastError());
  VG_HIP(hipcub::DeviceScan::ExclusiveSum((char*)runs.p + o_tmp, scan_tb, run_cnt, run_off, (int)cells, s));
  {
    int edge[65];  // the scan at every (slot, region) boundary, and the total
    for (int q = 0; q <= 2 * d.W; q++)
      VG_HIP(hipMemcpyAsync(&edge[q], run_off + (size_t)q * un, sizeof(int), hipMemcpyDeviceToHost, s));
    VG_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < d.W; k++) {
      d.ord0[k] = edge[2 * k + 1] - edge[2 * k];
      d.arena[k] = d.arena[k] ? d.cap_wp + (edge[2 * k + 2] - edge[2 * k + 1]) : 0;  // (never inserted: no runs)
    }
  }
  if (t_ms) t_ms[0] = now_ms() - t0;
  t0 = now_ms();
  // the image
  std::vector<unsigned char> blob;
  host_ckpt_blob(ctx, blob);
  Layout L;
  build_layout(ctx, d, blob.size(), nullptr, true, L);  // sizes first
  Scratch img;
  CK_ALLOC(img, L.image_bytes, "image");
  L = Layout();
  build_layout(ctx, d, blob.size(), (char*)img.p, true, L);
  VG_HIP(hipMemsetAsync(img.p, 0, L.image_bytes, s));  // the padding between sections
  VG_TRY(run_copy(ctx, L, who));
  const CkptSec* s_id = nullptr;
  const CkptSec* s_key = nullptr;
  const CkptSec* s_host = nullptr;
  const CkptSec* s_ord = nullptr;
  const CkptSec* s_lseg = nullptr;
  for (const CkptSec& q : L.sec) {
    if (q.id == kSecWpOrd) s_ord = &q;
    if (q.id == kSecLseg) s_lseg = &q;
    if (q.id == kSecRootId) s_id = &q;
    if (q.id == kSecRootKey) s_key = &q;
    if (q.id == kSecHost) s_host = &q;
  }
  if (d.n_nodes > 0)
    k_ckpt_runs_pack<<<grid_for((long)d.W * d.n_nodes), kBlock, 0, s>>>(m, d.n_nodes, run_off, (long)s_ord->count,
                                                                       (int*)((char*)img.p + s_ord->off),
                                                                       (uint64_t*)((char*)img.p + s_lseg->off));
  VG_HIP(hipGetLastError());
  if (d.n_roots > 0) {
    size_t tb = 0;
    int end_bit = 1;
    while ((1L << end_bit) <= (long)d.n_nodes) end_bit++;
    VG_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint64_t*)nullptr,
                                              (uint64_t*)nullptr, d.n_roots, 0, end_bit, s));
    Scratch tmp;
    CK_ALLOC(tmp, tb, "sort scratch");
    VG_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, (const uint32_t*)(rp + o_ids), (uint32_t*)((char*)img.p + s_id->off),
                                              (const uint64_t*)(rp + o_keys), (uint64_t*)((char*)img.p + s_key->off),
                                              d.n_roots, 0, end_bit, s));
    VG_HIP(hipStreamSynchronize(s));
  }
  if (!blob.empty())
    VG_HIP(hipMemcpyAsync((char*)img.p + s_host->off, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
  std::vector<uint64_t> sums(L.sec.size());
  VG_TRY(run_sums(ctx, (const unsigned char*)img.p, L.sec, sums.data(), who));
  for (size_t i = 0; i < L.sec.size(); i++) L.sec[i].sum = sums[i];
  if (t_ms) t_ms[1] = now_ms() - t0;
  t0 = now_ms();
  // header + image in one pinned buffer, one D2H copy
  const uint32_t nsec = (uint32_t)L.sec.size();
  const uint64_t hb = ckpt_head_bytes(nsec), total = hb + L.image_bytes;
  PinBuf pin;
  {
    const hipError_t e = hipHostMalloc(&pin.p, total, hipHostMallocDefault);
    if (e != hipSuccess) {
      pin.p = nullptr;
      ctx->err = std::string(who) + ": pinned buffer (" + std::to_string(total >> 20) + " MiB): " + hipGetErrorString(e);
      return VG_E_HIP;
    }
  }
  unsigned char* f = (unsigned char*)pin.p;
  memset(f, 0, hb);
  CkptHead h;
  memset(&h, 0, sizeof(h));
  memcpy(h.magic, kCkptMagic, 8);
  h.version = kCkptVersion;
  h.nsec = nsec;
  h.cfg_bytes = sizeof(vg_config);
  h.head_bytes = (uint32_t)hb;
  h.image_bytes = L.image_bytes;
  h.dims = d;
  memcpy(f, &h, sizeof(h));
  memcpy(f + sizeof(h), &ctx->cfg, sizeof(vg_config));
  memcpy(f + sizeof(h) + sizeof(vg_config), L.sec.data(), nsec * sizeof(CkptSec));
  h.head_sum = ckpt_head_sum(f, hb);
  memcpy(f, &h, sizeof(h));
  if (L.image_bytes > 0) VG_HIP(hipMemcpyAsync(f + hb, img.p, L.image_bytes, hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  if (t_ms) t_ms[2] = now_ms() - t0;
  t0 = now_ms();
  FILE* fp = fopen(path, "wb");
  if (!fp) {
    ctx->err = std::string(who) + ": cannot open " + path;
    return VG_E_ARG;
  }
  const size_t wr = fwrite(f, 1, total, fp);
  const int cl = fclose(fp);
  if (wr != total || cl != 0) {
    ctx->err = std::string(who) + ": short write to " + path;
    return VG_E_ARG;
  }
  if (t_ms) t_ms[3] = now_ms() - t0;
  if (bytes) *bytes = (long long)total;
  return VG_OK;
}

// t_ms (may be null): [0] file read + table checks, [1] host -> device, [2] checksum, [3] reset + unpack + hash rebuild
int checkpoint_load(vg_ctx* ctx, const char* path, double* t_ms) {
  const char* who = "vg_checkpoint_load";
  VG_TRY(host_ckpt_allowed(ctx, who, false));
  double t0 = now_ms();
  // the file into pinned memory
  FILE* fp = fopen(path, "rb");
  if (!fp) {
    ctx->err = std::string(who) + ": cannot open " + path;
    return VG_E_ARG;
  }
  fseek(fp, 0, SEEK_END);
  const long flen = ftell(fp);
  fseek(fp, 0, SEEK_SET);
  PinBuf pin;
  if (flen > 0 && hipHostMalloc(&pin.p, (size_t)flen, hipHostMallocDefault) != hipSuccess) {
    pin.p = nullptr;
    fclose(fp);
    ctx->err = std::string(who) + ": pinned buffer";
    return VG_E_HIP;
  }
  const size_t rd = flen > 0 ? fread(pin.p, 1, (size_t)flen, fp) : 0;
  fclose(fp);
  if (flen < 0 || rd != (size_t)flen) {
    ctx->err = std::string(who) + ": cannot read " + path;
    return VG_E_ARG;
  }
  const unsigned char* f = (const unsigned char*)pin.p;
  // 1-3: magic and version, the configuration, the section table and the file length
  CkptView v;
  std::string why;
  if (ckpt_validate(f, (uint64_t)flen, &ctx->cfg, &v, &why) != 0) {
    ctx->err = std::string(who) + ": " + why;
    return VG_E_ARG;
  }
  const CkptDims& d = v.head.dims;
  DevMap& m = ctx->map;
  if (d.cap_wp != m.cap_wp) {  // a layout parameter, not a capacity: the leaf runs' starts count from it
    ctx->err = std::string(who) + ": checkpoint rejected: config (max_points_per_scan " + std::to_string(d.cap_wp) +
               " in the file, " + std::to_string(m.cap_wp) + " here)";
    return VG_E_ARG;
  }
  if (t_ms) t_ms[0] = now_ms() - t0;
  t0 = now_ms();
  // 4: the checksums, recomputed on the device over the uploaded image
  hipStream_t s = ctx->stream;
  Scratch img;
  CK_ALLOC(img, v.head.image_bytes, "image");
  if (v.head.image_bytes > 0)
    VG_HIP(hipMemcpyAsync(img.p, f + v.head.head_bytes, v.head.image_bytes, hipMemcpyHostToDevice, s));
  VG_HIP(hipStreamSynchronize(s));
  if (t_ms) t_ms[1] = now_ms() - t0;
  t0 = now_ms();
  std::vector<uint64_t> sums(v.sec.size());
  VG_TRY(run_sums(ctx, (const unsigned char*)img.p, v.sec, sums.data(), who));
  for (size_t i = 0; i < v.sec.size(); i++)
    if (sums[i] != v.sec[i].sum) {
      ctx->err = std::string(who) + ": checkpoint rejected: checksum of section " + ckpt_name(v.sec[i].id);
      return VG_E_ARG;
    }
  if (t_ms) t_ms[2] = now_ms() - t0;
  t0 = now_ms();
  // the layout this context gives the same dimensions must be the file's
  Layout L;
  const CkptSec* s_host = v.find(kSecHost);
  build_layout(ctx, d, s_host->bytes, (char*)img.p, false, L);
  bool same = L.sec.size() == v.sec.size() && L.image_bytes == v.head.image_bytes;
  for (size_t i = 0; same && i < L.sec.size(); i++)
    same = L.sec[i].id == v.sec[i].id && L.sec[i].off == v.sec[i].off && L.sec[i].bytes == v.sec[i].bytes;
  if (!same) {
    ctx->err = std::string(who) + ": checkpoint rejected: section table (not this version's layout)";
    return VG_E_ARG;
  }
  void* snap = nullptr;
  if (host_ckpt_parse(ctx, f + v.head.head_bytes + s_host->off, s_host->bytes, &snap) != VG_OK) {
    ctx->err = std::string(who) + ": checkpoint rejected: host section malformed";
    return VG_E_ARG;
  }
  // 5: capacity
  std::string cap_err;
  if (d.n_nodes > m.cap_nodes) cap_err = "max_nodes " + std::to_string(m.cap_nodes) + " < " + std::to_string(d.n_nodes) + " nodes";
  else if (d.n_fix > m.cap_fix) cap_err = "max_fix_points " + std::to_string(m.cap_fix) + " < " + std::to_string(d.n_fix) + " points";
  else if (d.n_roots >= m.hash_mask) cap_err = "root hash (2^hash_log2) too small for " + std::to_string(d.n_roots) + " roots";
  if (!cap_err.empty()) {
    host_ckpt_drop(snap);
    ctx->err = std::string(who) + ": checkpoint rejected: capacity (" + cap_err + ")";
    return VG_E_CAPACITY;
  }
  // ---- every check passed: from here the context is rewritten
  int r = vg_reset(ctx);
  if (r == VG_OK) r = run_copy(ctx, L, who);
  if (r != VG_OK) {
    host_ckpt_drop(snap);
    return r;
  }
  auto fail = [&](int code) {
    host_ckpt_drop(snap);
    return code;
  };
  // wpn and the arena cursors (the header's dimensions)
  hipError_t e = hipMemcpyAsync(m.wpn, d.wpn, sizeof(d.wpn), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(m.arena, d.arena, sizeof(d.arena), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) {
    ctx->err = std::string(who) + ": " + hipGetErrorString(e);
    return fail(VG_E_HIP);
  }
  // the root hash, rebuilt for this context's table size
  if (d.n_nodes > 0) {
    const size_t un = (size_t)d.n_nodes;
    Scratch hb;
    const size_t o_pos = (un * 8 + 255) & ~size_t(255), o_cnt = (o_pos + un * 4 + 255) & ~size_t(255);
    {
      const hipError_t e2 = hb.reserve(o_cnt + 256);
      if (e2 != hipSuccess) {
        ctx->err = std::string(who) + ": hash scratch: " + hipGetErrorString(e2);
        return fail(VG_E_HIP);
      }
    }
    char* b = (char*)hb.p;
    int bad = 0;
    e = hipMemsetAsync(b + o_pos, 0xff, un * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(b + o_cnt, 0, 256, s);
    if (e == hipSuccess && d.n_roots > 0) {
      k_ckpt_hash_seed<<<grid_for(d.n_roots), kBlock, 0, s>>>(
          m.hash_mask, d.n_nodes, d.n_roots, (const int*)((char*)img.p + v.find(kSecRootId)->off),
          (const uint64_t*)((char*)img.p + v.find(kSecRootKey)->off), (uint64_t*)b, (int*)(b + o_pos),
          (int*)(b + o_cnt + 128));
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, b + o_cnt + 128, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
      ctx->err = std::string(who) + ": " + hipGetErrorString(e);
      return fail(VG_E_HIP);
    }
    if (bad) {
      ctx->err = std::string(who) + ": root pairs out of order";
      return fail(VG_E_STATE);
    }
    r = map_hash_place(ctx, d.n_nodes, d.n_roots, (const uint64_t*)b, (int*)(b + o_pos), (int*)(b + o_cnt), who);
    if (r != VG_OK) return fail(r);
  }
  e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    ctx->err = std::string(who) + ": " + hipGetErrorString(e);
    return fail(VG_E_HIP);
  }
  host_ckpt_install(ctx, snap);
  ctx->mk_keep = true;  // NodeHdr::mk came with the records (markers.hip markers_enable)
  if (t_ms) t_ms[3] = now_ms() - t0;
  return VG_OK;
}

}  // namespace vg
