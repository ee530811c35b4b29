// fleet_host.cpp — the fleet: B trackers attached to one owner's map (vg_map_attach)
// stepped together, one frozen scan each per step, in ten launches on one
// stream for any B (fleet.hip). The multi-sequence mode (multi.cpp) steps B
// full pipelines on their own streams and is bounded by the hardware queues; a
// frozen scan is host propagation, an optional deskew, the IEKF and a
// publication, and it never writes the map, so here the B scans share launches.
//
// Host side of one step, per participating tracker: what frozen_step
// (pipeline.cpp) runs ahead of the device — stage_propagate on the host path,
// which absorbs the tracker's previous publication, and the per-tracker deskew
// launch where per-point times are given — then the opening packed into the
// tracker's host-mapped block (FleetIn), and after the launches what
// stage_finish leaves behind: a pending publication the tracker's accessors
// absorb as they do a lone scan's. Every host wait is a wait on a tracker's own
// publication block.
#include <cstring>
#include <vector>

#include "vg_host.h"

namespace {
// The host-mapped blocks are a ring of steps: a block is rewritten kRing steps
// after the launches that read it. Before that the host makes sure those
// launches are done, by the publication of one tracker that took part in them
// (in order on the one stream, the publication is the step's last kernel).
constexpr int kRing = 4;
struct SlotUse {
  int tracker = -1, seq2 = 0;  // a participant of the step that last used the slot, its counter publication
};
}  // namespace

struct vg_fleet {
  vg_ctx* owner = nullptr;
  std::vector<vg_ctx*> ctx;
  hipStream_t stream = nullptr;
  std::vector<hipStream_t> own;   // each tracker's own stream (restored on destroy)
  std::vector<char> split;        // its IEKF overlap / downsample stream settings (vg_multi_create's bits)
  vg::FleetIn* h_in = nullptr;    // kRing x B blocks, host-mapped
  vg::FleetIn* d_in = nullptr;
  vg::DevBuf<vg::FleetTab> d_tab;  // B entries, device
  vg::DevBuf<int> d_act;           // B active flags, device
  SlotUse use[kRing];
  long step = 0;
  int nb = 0;                     // the IEKF grid per tracker
  int rc = VG_OK;                 // a failed step: the fleet is out of step and stays refused
  std::string err;
};

using namespace vg;

static int fleet_fail(vg_fleet* f, vg_ctx* c, int r) {
  if (f->rc == VG_OK) f->rc = r;
  if (c && c != f->ctx[0]) f->ctx[0]->err = c->err;  // (vg_last_error of the first tracker names it)
  return r;
}

extern "C" {

int vg_fleet_create(vg_ctx* owner, vg_ctx** trackers, int B, vg_fleet** out) {
  if (!owner || !trackers || B < 1 || !out) return VG_E_ARG;
  *out = nullptr;
  for (int b = 0; b < B; b++) {
    vg_ctx* c = trackers[b];
    if (!c) return VG_E_ARG;
    for (int a = 0; a < b; a++)
      if (trackers[a] == c) return VG_E_ARG;
    const char* why = c->view_of != owner ? "tracker is not attached to the owner (vg_map_attach)"
                      : c->fleet          ? "tracker already belongs to a fleet"
                      : hp(c)->in_scan    ? "tracker is inside a scan (vg_step_end first)"
                      : c->cap.max_points_per_scan != trackers[0]->cap.max_points_per_scan
                          ? "trackers differ in max_points_per_scan (one IEKF grid serves all)"
                          : nullptr;
    if (why) {
      c->err = std::string("vg_fleet_create: ") + why;
      owner->err = c->err;
      return VG_E_STATE;
    }
  }
  vg_ctx* ctx = owner;  // (VG_HIP reports into the owner)
  VG_HIP(hipSetDevice(owner->device));
  for (int b = 0; b < B; b++) VG_TRY(host_sync(trackers[b]));
  vg_fleet* f = new vg_fleet();
  f->owner = owner;
  f->ctx.assign(trackers, trackers + B);
  f->nb = iekf_grid(trackers[0]);
  auto fail = [&](hipError_t e) {
    owner->err = std::string("vg_fleet_create: ") + hipGetErrorString(e);
    vg_fleet_destroy(f);
    return VG_E_HIP;
  };
  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking)) != hipSuccess) return fail(e);
  const size_t in_bytes = (size_t)kRing * B * sizeof(FleetIn);
  if ((e = hipHostMalloc((void**)&f->h_in, in_bytes, hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess ||
      (e = hipHostGetDevicePointer((void**)&f->d_in, f->h_in, 0)) != hipSuccess)
    return fail(e);
  memset(f->h_in, 0, in_bytes);
  if ((e = f->d_tab.reserve(B)) != hipSuccess || (e = f->d_act.reserve(B)) != hipSuccess ||
      (e = hipMemset(f->d_act, 0, B * sizeof(int))) != hipSuccess)
    return fail(e);
  std::vector<FleetTab> tab(B);
  for (int b = 0; b < B; b++) {
    vg_ctx* c = trackers[b];
    tab[b] = FleetTab{c->st, c->wk.iekf_cache, c->wk.partials, c->d_pub, f->d_act + b};
    // a fleet step runs no downsample: the last one's count does not outlive the switch (vg_scan_points)
    if ((e = hipMemset(c->ds.hflags + 1, 0, sizeof(int))) != hipSuccess) return fail(e);
  }
  if ((e = hipMemcpy(f->d_tab, tab.data(), B * sizeof(FleetTab), hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
  // every tracker on the fleet's one stream; its own downsample and IEKF
  // streams are not made while it is here (vg_multi_create's arrangement)
  f->own.resize(B);
  f->split.assign(B, 0);
  for (int b = 0; b < B; b++) {
    vg_ctx* c = trackers[b];
    f->split[b] = (char)((c->overlap_iekf ? 1 : 0) | (c->want_ds_stream ? 2 : 0));
    c->overlap_iekf = false;
    c->want_ds_stream = false;
    if (c->stream_ds && c->stream_ds != c->stream) {
      (void)hipStreamSynchronize(c->stream_ds);
      (void)hipStreamDestroy(c->stream_ds);
    }
    (void)hipStreamSynchronize(c->stream);
    f->own[b] = c->stream;
    c->stream = f->stream;
    c->stream_ds = f->stream;
    c->fleet = f;
  }
  *out = f;
  return VG_OK;
}

// Queue every participating scan or none: the records are checked, and every
// tracker's deferred error looked at, before anything is propagated or enqueued.
int vg_fleet_step_dev(vg_fleet* f, const vg_scan_dev* scans) {
  if (!f || !scans) return VG_E_ARG;
  if (f->rc != VG_OK) return f->rc;
  const int B = (int)f->ctx.size();
  int active = 0;
  for (int b = 0; b < B; b++) {
    const vg_scan_dev& sc = scans[b];
    vg_ctx* c = f->ctx[b];
    if (sc.n < 0) continue;
    if ((sc.n > 0 && (!sc.d_x || !sc.d_y || !sc.d_z)) || sc.m < 0 || (sc.m > 0 && !sc.imu)) {
      c->err = "vg_fleet_step_dev: bad scan record (a null plane with n > 0, or no IMU samples with m > 0)";
      return VG_E_ARG;
    }
    if (sc.n > c->cap.max_points_per_scan) {
      c->err = "scan larger than max_points_per_scan";
      return VG_E_CAPACITY;
    }
    if (hp(c)->sticky != VG_OK) return hp(c)->sticky;
    active++;
  }
  if (active == 0) return VG_OK;
  vg_ctx* ctx = f->ctx[0];  // (VG_HIP reports into the first tracker)
  VG_HIP(hipSetDevice(f->owner->device));
  const int slot = (int)(f->step % kRing);
  if (f->use[slot].tracker >= 0) {  // the launches that read this slot's blocks, kRing steps ago, are done
    vg_ctx* c = f->ctx[f->use[slot].tracker];
    const int r = pub_wait(c, &c->h_pub->seq2, f->use[slot].seq2, "fleet step");
    if (r != VG_OK) return fleet_fail(f, c, r);
    f->use[slot].tracker = -1;
  }
  FleetIn* in = f->h_in + (size_t)slot * B;
  for (int b = 0; b < B; b++) {
    const vg_scan_dev& sc = scans[b];
    vg_ctx* c = f->ctx[b];
    FleetIn& a = in[b];
    a.active = 0;
    if (sc.n < 0) continue;
    HostPipe* P = hp(c);
    int r = stage_propagate(c, sc.imu, sc.m, sc.pcl_beg_time, sc.pcl_end_time);
    const float *x = sc.d_x, *y = sc.d_y, *z = sc.d_z;
    if (r == VG_OK && sc.d_time) {  // the per-tracker deskew launch, on the fleet stream like everything of the tracker's
      r = stage_deskew(c, sc.d_x, sc.d_y, sc.d_z, sc.d_intensity, sc.d_time, sc.n);
      x = c->d_x, y = c->d_y, z = c->d_z;
    }
    if (r != VG_OK) {
      // Past the record checks a step cannot be taken back: the trackers up to b have propagated.
      // Their opened scans are abandoned (nothing of them was launched), so no tracker is left
      // inside a scan, and the fleet stays refused: it is out of step (vina_gpu.h)
      for (int a2 = 0; a2 <= b; a2++) {
        HostPipe* Q = hp(f->ctx[a2]);
        if (a2 == b || in[a2].active) Q->in_scan = Q->begin_pending = false;
        in[a2].active = 0;
      }
      return fleet_fail(f, c, r);
    }
    memcpy(a.xc, P->begin_xc, sizeof(a.xc));  // the opening stage_propagate left pending rides in the block
    P->begin_pending = false;
    a.x = x;
    a.y = y;
    a.z = z;
    a.n = sc.n;
    a.win_count = P->win_count;
    a.seq1 = ++c->pub_seq;
    a.seq2 = ++c->pub_seq;
    a.active = 1;
  }
  std::string lerr;
  const int r = fleet_launch(f->stream, hp(f->owner)->mpd, f->owner->map, f->d_in + (size_t)slot * B, f->d_tab, B,
                             f->nb, f->ctx[0]->iekf_prefetch, &lerr);
  if (r != VG_OK) {
    f->ctx[0]->err = lerr;
    for (int b = 0; b < B; b++)
      if (in[b].active) hp(f->ctx[b])->in_scan = hp(f->ctx[b])->begin_pending = false;
    return fleet_fail(f, nullptr, r);
  }
  // the end of the scan (stage_finish): the publications are the step's last kernel
  for (int b = 0; b < B; b++) {
    if (!in[b].active) continue;
    vg_ctx* c = f->ctx[b];
    HostPipe* P = hp(c);
    P->n_raw = scans[b].n;
    P->cur.st.n_raw = scans[b].n;
    P->cur.ev_n = 0;
    P->cur.frozen = true;
    P->cur.n_ds = 0;  // no downsample in a fleet step (vina_gpu.h)
    P->cur.seq1 = in[b].seq1;
    P->cur.seq2 = in[b].seq2;
    P->published = true;
    P->pend.push_back(P->cur);
    P->in_scan = false;
    P->first = false;
    f->use[slot].tracker = b;
    f->use[slot].seq2 = in[b].seq2;
  }
  f->step++;
  return VG_OK;
}

int vg_fleet_sync(vg_fleet* f) {
  if (!f) return VG_E_ARG;
  int rc = f->rc;
  for (vg_ctx* c : f->ctx) {
    const int r = host_sync(c);    // completes every enqueued scan of the tracker
    if (r != VG_OK && rc == VG_OK) rc = r;
  }
  return rc;
}

void vg_fleet_destroy(vg_fleet* f) {
  if (!f) return;
  if (f->stream) (void)hipStreamSynchronize(f->stream);
  // each tracker back as it came: its own stream, its downsample stream made again on the next scan
  for (size_t b = 0; b < f->own.size(); b++) {
    vg_ctx* c = f->ctx[b];
    c->stream = f->own[b];
    c->stream_ds = c->stream;
    if (f->split[b] & 2) c->want_ds_stream = true;
    if (f->split[b] & 1) c->overlap_iekf = true;
    c->fleet = nullptr;
  }
  if (f->h_in) (void)hipHostFree(f->h_in);
  if (f->stream) (void)hipStreamDestroy(f->stream);
  delete f;
}

}  // extern "C"
