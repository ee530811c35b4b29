// places_host.cpp — the place index behind the C-ABI (vina_gpu.h "Place
// index"): the state checks, the drain of outstanding work, the mutex that
// serialises the calls into one index, the top-k selection, and global
// relocalisation on top of vg_relocalize's own routine (the kernels and the
// index's memory: places.hip).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "vg_host.h"

namespace vg {

static vg_ctx* map_owner(vg_ctx* ctx) { return ctx->view_of ? ctx->view_of : ctx; }

static int state_err(vg_ctx* ctx, const char* who, const char* why) {
  ctx->err = std::string(who) + ": " + why;
  return VG_E_STATE;
}

// rows ex, ey, up from the gravity of the context's state
static void place_frame(const V3& g, double* f) {
  V3 up = scl(g, -1.0);
  const double gn = norm3(up);
  up = gn > 0 ? scl(up, 1.0 / gn) : v3(0, 0, 1);
  const V3 ref = std::fabs(up[0]) < 0.9 ? v3(1, 0, 0) : v3(0, 1, 0);
  V3 ex = sub(ref, scl(up, dot3(ref, up)));
  ex = scl(ex, 1.0 / norm3(ex));
  const V3 ey = cross3(up, ex);
  for (int j = 0; j < 3; j++) {
    f[j] = ex[j];
    f[3 + j] = ey[j];
    f[6 + j] = up[j];
  }
}

// the median, over the places (at most 1024 of them, evenly strided), of the distance to the nearest other
// place in the ex-ey plane
static double nn_spacing(const std::vector<double>& pos, int M, const double* f) {
  if (M < 2) return 0.0;
  std::vector<double> u((size_t)M), v((size_t)M), d;
  for (int i = 0; i < M; i++) {
    const double* p = &pos[3 * (size_t)i];
    u[i] = p[0] * f[0] + p[1] * f[1] + p[2] * f[2];
    v[i] = p[0] * f[3] + p[1] * f[4] + p[2] * f[5];
  }
  const int stride = (M + 1023) / 1024;
  for (int i = 0; i < M; i += stride) {
    double b = HUGE_VAL;
    for (int j = 0; j < M; j++) {
      if (j == i) continue;
      const double du = u[i] - u[j], dv = v[i] - v[j], q = du * du + dv * dv;
      if (q < b) b = q;
    }
    d.push_back(std::sqrt(b));
  }
  std::nth_element(d.begin(), d.begin() + d.size() / 2, d.end());
  return d[d.size() / 2];
}

int host_places_build(vg_ctx* ctx, const double* positions, int M, const vg_places_params* prm) {
  const char* who = "vg_places_build";
  std::lock_guard<std::mutex> lock(ctx->places_mu);
  if (ctx->mapping) return state_err(ctx, who, "mapping is on (vg_set_mapping(ctx, 0) first)");
  if (sharded(ctx) || ctx->shard.world > 1) return state_err(ctx, who, "the context is sharded");
  if (hp(ctx)->in_scan) return state_err(ctx, who, "the context is inside a scan (vg_step_end first)");
  if (ctx->view_of) return state_err(ctx, who, "the context is attached to another context's map (build on the owner)");
  int A = 0, E = 0;
  if (places_prm_ok(prm, &A, &E) != VG_OK) {
    ctx->err = std::string(who) + ": bad parameters (n_az <= 256, n_el <= 32, n_az * n_el <= 4096, el_min < el_max)";
    return VG_E_ARG;
  }
  if ((long long)M * A * E >= (1ll << 30)) {
    ctx->err = std::string(who) + ": M * n_az * n_el reaches 2^30";
    return VG_E_ARG;
  }
  for (size_t i = 0; i < (size_t)M * 3; i++)
    if (!std::isfinite(positions[i])) {
      ctx->err = std::string(who) + ": a position is not finite";
      return VG_E_ARG;
    }
  VG_TRY(host_quiesce(ctx));
  PlaceIndex* I = new PlaceIndex();
  memset(&I->prm, 0, sizeof(I->prm));
  if (prm) I->prm = *prm;
  I->M = M;
  I->pos.assign(positions, positions + (size_t)M * 3);
  place_frame(hp(ctx)->x_curr.g, I->frame);
  I->spacing = nn_spacing(I->pos, M, I->frame);
  const int r = places_build_dev(ctx, I, hp(ctx)->mpd);
  if (r != VG_OK) {
    delete I;
    return r;
  }
  delete ctx->places;  // replaced only once the new one stands
  ctx->places = I;
  return VG_OK;
}

int host_places_end(vg_ctx* ctx) {
  const char* who = "vg_places_end";
  // a call in flight on another thread finishes first; one that waits for the lock finds no index (VG_E_STATE)
  std::lock_guard<std::mutex> lock(ctx->places_mu);
  if (ctx->view_of) return state_err(ctx, who, "the context is attached: the index belongs to the map's owner");
  if (!ctx->places) return state_err(ctx, who, "the context has no place index");
  PlaceIndex* I = ctx->places;
  ctx->places = nullptr;
  delete I;
  return VG_OK;
}

int host_places_info(vg_ctx* ctx, int* M, int* n_valid, uint16_t* desc, int32_t* hit_bins) {
  vg_ctx* owner = map_owner(ctx);
  std::lock_guard<std::mutex> lock(owner->places_mu);
  PlaceIndex* I = owner->places;  // read under the lock: vg_places_end on another thread cannot free it under this call
  if (!I) return state_err(ctx, "vg_places_info", "the map this context reads has no place index");
  if (M) *M = I->M;
  if (n_valid) *n_valid = I->n_valid;
  if (hit_bins) memcpy(hit_bins, I->hit.data(), (size_t)I->M * sizeof(int));
  if (desc) VG_HIP(hipMemcpy(desc, I->d_desc, (size_t)I->M * I->A * I->E * sizeof(uint16_t), hipMemcpyDeviceToHost));
  return VG_OK;
}

static int places_allowed(vg_ctx* ctx, const char* who) {
  if (ctx->shard.world > 1) return state_err(ctx, who, "the context is sharded (world > 1)");
  return host_quiesce(ctx);
}

static void level_of(vg_ctx* ctx, const double* R_level9, double* R) {
  if (R_level9) memcpy(R, R_level9, 72);
  else memcpy(R, hp(ctx)->x_curr.R.a, 72);  // the host mirror, current after the drain
}

int host_places_scan(vg_ctx* ctx, const float* xyz, int n, const double* R_level9, uint16_t* desc,
                     int32_t* n_per_bin) {
  const char* who = "vg_places_scan";
  VG_TRY(places_allowed(ctx, who));
  double R[9];
  level_of(ctx, R_level9, R);
  vg_ctx* owner = map_owner(ctx);
  std::lock_guard<std::mutex> lock(owner->places_mu);
  PlaceIndex* I = owner->places;
  if (!I) return state_err(ctx, who, "the map this context reads has no place index (vg_places_build on its owner)");
  return places_scan_dev(ctx, I, hp(ctx)->mpd, xyz, n, R, desc, n_per_bin, nullptr);
}

// out: up to top_k records; frame9 / spacing / n_az (may be null): the index's, for the caller's poses and window
int host_places_query(vg_ctx* ctx, const float* xyz, int n, const double* R_level9, int top_k,
                      vg_place_candidate* out, int* n_out, int32_t* scores_all, double* frame9, double* spacing,
                      int* n_az) {
  const char* who = "vg_places_query";
  VG_TRY(places_allowed(ctx, who));
  double R[9];
  level_of(ctx, R_level9, R);
  vg_ctx* owner = map_owner(ctx);
  std::lock_guard<std::mutex> lock(owner->places_mu);
  PlaceIndex* I = owner->places;
  if (!I) return state_err(ctx, who, "the map this context reads has no place index (vg_places_build on its owner)");
  if (frame9) memcpy(frame9, I->frame, 72);
  if (spacing) *spacing = I->spacing;
  if (n_az) *n_az = I->A;
  int nv = 0;
  VG_TRY(places_scan_dev(ctx, I, hp(ctx)->mpd, xyz, n, R, nullptr, nullptr, &nv));
  std::vector<int> best((size_t)I->M * 4);
  VG_TRY(places_match_dev(ctx, I, best.data(), scores_all));
  *n_out = 0;
  if (n == 0 || nv == 0) return VG_OK;
  struct Rec {
    int score, place, shift;
  };
  std::vector<Rec> rec;
  rec.reserve((size_t)I->M * 2);
  for (int m = 0; m < I->M; m++)
    for (int k = 0; k < 2; k++) {
      const int s = best[4 * (size_t)m + 2 * k], sc = best[4 * (size_t)m + 2 * k + 1];
      if (s >= 0 && sc != INT_MAX) rec.push_back({sc, m, s});
    }
  const size_t keep = std::min((size_t)top_k, rec.size());
  std::partial_sort(rec.begin(), rec.begin() + keep, rec.end(), [](const Rec& a, const Rec& b) {
    if (a.score != b.score) return a.score < b.score;
    if (a.place != b.place) return a.place < b.place;
    return a.shift < b.shift;
  });
  for (size_t k = 0; k < keep; k++) {
    vg_place_candidate& c = out[k];
    c.place = rec[k].place;
    c.shift = rec[k].shift;
    c.score = rec[k].score;
    c.n_valid = nv;
    memcpy(c.pos, &I->pos[3 * (size_t)rec[k].place], 24);
    c.yaw = 2.0 * M_PI * rec[k].shift / I->A;
  }
  *n_out = (int)keep;
  return VG_OK;
}

int host_relocalize_global(vg_ctx* ctx, const float* xyz, int n, const double* R_level9, int top_k,
                           const vg_reloc_params* prm, int install, double* out_pose, vg_pose_score* out_score,
                           vg_place_candidate* out_place, int* ok) {
  const char* who = "vg_relocalize_global";
  if (hp(ctx)->in_scan) return state_err(ctx, who, "inside a scan (vg_step_end first)");
  top_k = std::min(top_k, 4096);  // (what is verified one by one; vina_gpu.h)
  std::vector<vg_place_candidate> cand((size_t)top_k);
  int nc = 0, A = 0;
  double f[9], spacing = 0.0, Rl[9];
  VG_TRY(host_places_query(ctx, xyz, n, R_level9, top_k, cand.data(), &nc, nullptr, f, &spacing, &A));
  level_of(ctx, R_level9, Rl);
  vg_reloc_params win;
  if (prm) {
    win = *prm;
  } else {
    memset(&win, 0, sizeof(win));
    win.half_xy = 0.5 * spacing;
    win.step_xy = 0.25;
    win.half_yaw = 1.5 * (2.0 * M_PI / A);
    win.step_yaw = (2.0 * M_PI / A) / 3.0;
  }
  const MP& mp = hp(ctx)->mpd;
  const V3 up = v3(f[6], f[7], f[8]);
  M3 R0;
  memcpy(R0.a, Rl, 72);
  *ok = 0;
  memset(out_pose, 0, 12 * sizeof(double));
  memcpy(out_pose, Rl, 72);
  vg_pose_score best;
  memset(&best, 0, sizeof(best));
  int won = -1;
  for (int k = 0; k < nc; k++) {
    // the candidate's pose: R = Rz_up(yaw) R_level, p = pos - R ext_t
    double guess[12], pose[12];
    const M3 R = mul(Exp(scl(up, cand[k].yaw)), R0);
    const V3 t = mv3(R, v3(mp.extt[0], mp.extt[1], mp.extt[2]));
    memcpy(guess, R.a, 72);
    for (int j = 0; j < 3; j++) guess[9 + j] = cand[k].pos[j] - t[j];
    vg_pose_score sc;
    int good = 0;
    VG_TRY(host_relocalize(ctx, xyz, n, guess, &win, 0, pose, &sc, &good));
    // a candidate that verifies beats one that does not; among equals vg_relocalize's ranking
    const bool first = won < 0, up_ok = good && !*ok, same = (good != 0) == (*ok != 0);
    if (first || up_ok || (same && reloc_better(sc, best))) {
      best = sc;
      won = k;
      *ok = good;
      memcpy(out_pose, pose, sizeof(pose));
    }
  }
  // The winner started a fraction of the places' spacing (and of their height) from the truth, and the
  // ranking may have picked an iterate short of the minimum (on the way the match set changes, and an
  // iterate can hold a few more matches than the fixed point it is heading for). The candidates decide the
  // basin; the pose reported is where the same refinement comes to rest in it: again from where it stands,
  // as a grid of one hypothesis, until it moves less than its own stopping rule (at most 4 times)
  for (int round = 0; round < 4 && *ok; round++) {
    vg_reloc_params one = win;
    one.half_xy = one.half_z = one.half_yaw = 0.0;
    one.refine_top = 1;
    double guess[12], pose[12];
    memcpy(guess, out_pose, sizeof(guess));
    vg_pose_score sc;
    int good = 0;
    VG_TRY(host_relocalize(ctx, xyz, n, guess, &one, 0, pose, &sc, &good));
    if (!good) break;
    M3 Ra, Rb;
    memcpy(Ra.a, guess, 72);
    memcpy(Rb.a, pose, 72);
    const double dr = norm3(Log(mul(tr(Ra), Rb)));
    const double dp = norm3(v3(pose[9] - guess[9], pose[10] - guess[10], pose[11] - guess[11]));
    best = sc;
    memcpy(out_pose, pose, sizeof(pose));
    if (dr < 1e-7 && dp < 1e-6) break;
  }
  if (out_score) *out_score = best;
  if (out_place) {
    memset(out_place, 0, sizeof(*out_place));
    if (won >= 0) *out_place = cand[won];
    else out_place->place = out_place->shift = -1;
  }
  if (*ok && install) VG_TRY(reloc_install(ctx, out_pose));
  return VG_OK;
}

}  // namespace vg

extern "C" {
int vg_places_dirs(const vg_places_params* prm, double* out, int cap, int* count) {
  if (!count || cap < 0) return VG_E_ARG;
  return vg::places_dirs(prm, out, cap, count);
}
int vg_places_build(vg_ctx* ctx, const double* positions, int M, const vg_places_params* prm) {
  if (!ctx || !positions || M <= 0) return VG_E_ARG;
  return vg::host_places_build(ctx, positions, M, prm);
}
int vg_places_info(vg_ctx* ctx, int* M, int* n_valid, uint16_t* desc, int32_t* hit_bins) {
  if (!ctx) return VG_E_ARG;
  return vg::host_places_info(ctx, M, n_valid, desc, hit_bins);
}
int vg_places_scan(vg_ctx* ctx, const float* xyz, int n, const double* R_level9, uint16_t* desc, int32_t* n_per_bin) {
  if (!ctx || n < 0 || (n > 0 && !xyz) || n > ctx->cap.max_points_per_scan) return VG_E_ARG;
  return vg::host_places_scan(ctx, xyz, n, R_level9, desc, n_per_bin);
}
int vg_places_query(vg_ctx* ctx, const float* xyz, int n, const double* R_level9, int top_k, vg_place_candidate* out,
                    int* n_out, int32_t* scores_all) {
  if (!ctx || n < 0 || (n > 0 && !xyz) || n > ctx->cap.max_points_per_scan || top_k <= 0 || !out || !n_out)
    return VG_E_ARG;
  return vg::host_places_query(ctx, xyz, n, R_level9, top_k, out, n_out, scores_all, nullptr, nullptr, nullptr);
}
int vg_places_end(vg_ctx* ctx) {
  if (!ctx) return VG_E_ARG;
  return vg::host_places_end(ctx);
}
int vg_relocalize_global(vg_ctx* ctx, const float* xyz, int n, const double* R_level9, int top_k,
                         const vg_reloc_params* prm, int install, double* out_pose, vg_pose_score* out_score,
                         vg_place_candidate* out_place, int* ok) {
  if (!ctx || n < 0 || (n > 0 && !xyz) || n > ctx->cap.max_points_per_scan || top_k <= 0 || !out_pose || !ok)
    return VG_E_ARG;
  return vg::host_relocalize_global(ctx, xyz, n, R_level9, top_k, prm, install, out_pose, out_score, out_place, ok);
}
}
