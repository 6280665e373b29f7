// dmi_capi_viewset.hip -- dmi_views_* of include/dmi.h: the resident view set (dmi_view_set.h).  The argument checks (all of them
// before the device is touched), the set's life cycle, the ingest of an add, and per step the pieces of whole views
// (view_set_rules.h): each piece runs the per-piece body its context-free counterpart runs -- every sequence of launches lives
// beside that entry point; the single launches of 8g's upload and finish passes are made here, on the set's own planes -- from D
// into the alternate plane, and the report kernels of view_set_kernels.hip behind it (run_pieces).  The planes change
// places when every piece has succeeded.  The checks the entries share with the context-free calls, the camera upload, the flip of
// a piece and the spans between events are dmi_depth_call.h's.  A failure's text is dmi_views_last_error(s)'s.
#include <algorithm>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "dmi_context.h"
#include "dmi_depth_call.h"
#include "dmi_view_set.h"
#include "view_set_kernels.h"

namespace dmi {

namespace {
thread_local std::string g_create_error;
}

int views_fail(dmi_view_set *s, int code, const std::string &msg) {
  if (s)
    s->err = msg;
  else
    g_create_error = msg;
  return code;
}

}  // namespace dmi

namespace {

namespace rules = dmi::view_set_rules;
int fail(dmi_view_set *s, int code, const std::string &msg) { return dmi::views_fail(s, code, msg); }
dmi_view_set *const kNoSet = nullptr;  // a failure without a set: the thread's last create failure

using dmi::finite_and_not_negative;

#define VS_HIP(s, call)                                                                             \
  do {                                                                                              \
    hipError_t e_ = (call);                                                                         \
    if (e_ != hipSuccess) {                                                                         \
      (void)hipGetLastError();                                                                      \
      return fail(s, e_ == hipErrorOutOfMemory ? DMI_ERR_OUT_OF_MEMORY : DMI_ERR_DEVICE,            \
                  std::string(#call) + ": " + hipGetErrorString(e_));                               \
    }                                                                                               \
  } while (0)

template <typename Body>
int guarded(dmi_view_set *s, const char *entry, Body &&body) noexcept {
  return dmi::guarded_by<dmi_view_set>(&dmi::views_fail, s, entry, static_cast<Body &&>(body));
}

hipError_t grow(dmi_view_set *s, dmi::DeviceBuffer &buffer, uint64_t bytes) { return dmi::grow_buffer(buffer, bytes, s->device_bytes); }

// what every entry opens with (`entry` ends in ": "): DMI_OK, or the refusal of a call without a set, of a set without views
int require_set(dmi_view_set *s, const std::string &entry) {
  return s ? DMI_OK : fail(kNoSet, DMI_ERR_INVALID_ARGUMENT, entry + "the set is null");
}
int require_views(dmi_view_set *s, const std::string &entry) {
  return s->n >= 1 ? DMI_OK : fail(s, DMI_ERR_INVALID_ARGUMENT, entry + "the set holds no views");
}

// what a consistency or bounds pass holds beside the set's planes: freed whatever way the pass ends
struct WholeSetScratch {
  dmi_view_set *s;
  ~WholeSetScratch() {
    (void)hipStreamSynchronize(s->stream);
    dmi::free_buffers({&s->flipped, &s->counts, &s->cameras, &s->state, &s->hist, &s->flags, &s->block_counts, &s->block_offsets},
                      s->device_bytes);
  }
};

// D changes, or the views do: the points of the last build describe neither any longer
void drop_points(dmi_view_set *s) {
  if (s->points.ptr || s->plane_rms.ptr) {
    (void)hipSetDevice(s->device);
    dmi::free_buffers({&s->points, &s->plane_rms}, s->device_bytes);
  }
  s->points_fitted = false;
  s->n_points = 0;
  s->points_current = false;
  s->points_thinned = false;
  s->points_filtered = false;
}

struct Pieces {
  size_t plane;  // pixels of a view
  int64_t per, count;
};
Pieces pieces_of(const dmi_view_set *s, int64_t n) {
  Pieces p;
  p.plane = (size_t)s->W * (size_t)s->H;
  p.per = rules::piece_views(s->piece_bytes, s->W, s->H, n);
  p.count = rules::piece_count(n, p.per);
  return p;
}

double *plane_of(const dmi_view_set *s, int which) { return s->plane[which].as<double>(); }
unsigned long long *counters_of(const dmi_view_set *s) { return s->counters.as<unsigned long long>(); }

int begin_step(dmi_view_set *s) {
  VS_HIP(s, hipSetDevice(s->device));
  VS_HIP(s, hipMemsetAsync(s->counters.ptr, 0, dmi::kVsCounters * sizeof(unsigned long long), s->stream));
  return DMI_OK;
}

// the piece's work is queued: wait for it and add the spans between `n_events` pass events and between the report's two
int end_piece(dmi_view_set *s, int n_events, double *pass_ms, double *report_ms) {
  VS_HIP(s, hipStreamSynchronize(s->stream));  // the scratch and the events are reused by the next piece
  VS_HIP(s, dmi::add_spans(s->events, n_events - 1, pass_ms, 0));
  VS_HIP(s, dmi::add_spans(s->report_events, 1, report_ms));
  return DMI_OK;
}

// every piece has succeeded: the counters come down, the planes change places, the report is written
int end_step(dmi_view_set *s, rules::Step step, double pass_ms, double report_ms, dmi_views_step_report *r) {
  unsigned long long c[dmi::kVsCounters];
  VS_HIP(s, hipMemcpyAsync(c, s->counters.ptr, sizeof(c), hipMemcpyDeviceToHost, s->stream));
  VS_HIP(s, hipStreamSynchronize(s->stream));
  drop_points(s);
  s->current ^= 1;
  s->steps += 1;
  s->last_report_kernel_ms = report_ms;
  if (r) {
    const rules::Report made = rules::make_report(step, {c[dmi::kVsValidBefore], c[dmi::kVsValidAfter], c[dmi::kVsDiffering],
                                                         c[dmi::kVsAuxSum], c[dmi::kVsRoots], c[dmi::kVsRootsKept]});
    r->valid_before = made.valid_before;
    r->valid_after = made.valid_after;
    r->changed = made.changed;
    r->groups = made.groups;
    r->groups_kept = made.groups_kept;
    r->aux_sum = made.aux_sum;
    r->kernel_ms = pass_ms;
  }
  return DMI_OK;
}

int create(int32_t device, int32_t W, int32_t H, dmi_view_set **out) {
  const std::string entry = "dmi_views_create: ";
  auto bad = [&](const std::string &what) { return fail(kNoSet, DMI_ERR_INVALID_ARGUMENT, entry + what); };
  if (!out) return bad("out is null");
  *out = nullptr;
  if (const char *what = dmi::side_refusal(W, H)) return bad(what);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return fail(kNoSet, DMI_ERR_DEVICE, entry + "no HIP device available");
  }
  if (device < 0 || device >= ndev) return bad("device ordinal out of range");
  dmi_view_set *s = new dmi_view_set;
  s->device = device;
  s->W = W;
  s->H = H;
  auto give_up = [&](hipError_t e, const char *what) {
    (void)hipGetLastError();
    const std::string msg = entry + what + ": " + hipGetErrorString(e);
    dmi_views_destroy(s);
    return fail(kNoSet, e == hipErrorOutOfMemory ? DMI_ERR_OUT_OF_MEMORY : DMI_ERR_DEVICE, msg);
  };
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return give_up(e, "hipSetDevice");
  e = hipDeviceGetAttribute(&s->compute_units, hipDeviceAttributeMultiprocessorCount, device);
  if (e != hipSuccess) return give_up(e, "hipDeviceGetAttribute");
  e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
  if (e != hipSuccess) return give_up(e, "hipStreamCreateWithFlags");
  for (hipEvent_t &ev : s->events)
    if ((e = hipEventCreate(&ev)) != hipSuccess) return give_up(e, "hipEventCreate");
  for (hipEvent_t &ev : s->report_events)
    if ((e = hipEventCreate(&ev)) != hipSuccess) return give_up(e, "hipEventCreate");
  if ((e = hipEventCreateWithFlags(&s->handed_over, hipEventDisableTiming)) != hipSuccess) return give_up(e, "hipEventCreate");
  if ((e = grow(s, s->counters, dmi::kVsCounters * sizeof(unsigned long long))) != hipSuccess) return give_up(e, "hipMalloc");
  *out = s;
  return DMI_OK;
}

int add(dmi_view_set *s, const double *depth, const double *best_cost, double threshold, const double *K4, const double *RT4, int32_t n) {
  const std::string entry = "dmi_views_add: ";
  if (const int rc = require_set(s, entry)) return rc;
  auto bad = [&](const std::string &what) { return fail(s, DMI_ERR_INVALID_ARGUMENT, entry + what); };
  if (!depth) return bad("depth is null");
  if (!K4) return bad("K4 is null");
  if (!RT4) return bad("RT4 is null");
  if (n < 1) return bad("n >= 1 required");
  if ((int64_t)s->n + n > 0x7fffffffLL) return bad("the set cannot hold more than 2^31 - 1 views");
  if (best_cost && threshold != threshold) return bad("threshold is NaN");
  const size_t plane = (size_t)s->W * (size_t)s->H, held = (size_t)s->n, total = held + (size_t)n;
  uint64_t resident = 0;
  if (!rules::resident_bytes(total, s->W, s->H, &resident)) return bad("the views' planes do not fit 64 bits of bytes");

  VS_HIP(s, hipSetDevice(s->device));
  // both planes hold `total` views, D keeps its contents: all or nothing
  if (!dmi::holds(s->plane[s->current], total * plane * 8)) {
    dmi::DeviceBuffer grown;
    hipError_t e = grow(s, grown, total * plane * 8);
    if (e == hipSuccess && held)
      e = hipMemcpyAsync(grown.ptr, s->plane[s->current].ptr, held * plane * 8, hipMemcpyDeviceToDevice, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) {
      dmi::free_buffers({&grown}, s->device_bytes);
      VS_HIP(s, e);
    }
    dmi::free_buffers({&s->plane[s->current]}, s->device_bytes);
    s->plane[s->current] = grown;
  }
  VS_HIP(s, grow(s, s->plane[s->current ^ 1], total * plane * 8));

  const Pieces p = pieces_of(s, n);
  // (two doubles of room: a staged piece stands as far from a 16-byte boundary as its place in D does)
  VS_HIP(s, grow(s, s->stage_depth, (uint64_t)p.per * plane * 8 + 16));
  if (best_cost) VS_HIP(s, grow(s, s->stage_cost, (uint64_t)p.per * plane * 8 + 16));
  VS_HIP(s, hipMemsetAsync(s->counters.ptr, 0, dmi::kVsCounters * sizeof(unsigned long long), s->stream));
  for (int64_t q = 0; q < p.count; ++q) {
    const rules::Piece piece = rules::piece_at(n, p.per, q);
    double *const dst = plane_of(s, s->current) + (held + (size_t)piece.first) * plane;
    const size_t shift = (size_t)((reinterpret_cast<uintptr_t>(dst) & 15) / 8), elems = (size_t)piece.count * plane;
    double *const up_depth = s->stage_depth.as<double>() + shift;
    double *const up_cost = best_cost ? s->stage_cost.as<double>() + shift : nullptr;
    VS_HIP(s, hipMemcpyAsync(up_depth, depth + (size_t)piece.first * plane, elems * 8, hipMemcpyHostToDevice, s->stream));
    if (best_cost)
      VS_HIP(s, hipMemcpyAsync(up_cost, best_cost + (size_t)piece.first * plane, elems * 8, hipMemcpyHostToDevice, s->stream));
    VS_HIP(s, dmi::launch_view_set_ingest(up_depth, up_cost, threshold, dst, elems, counters_of(s), s->compute_units, s->stream));
    VS_HIP(s, hipStreamSynchronize(s->stream));  // the stage buffers are reused by the next piece
  }
  s->h2d_plane_bytes += (uint64_t)n * plane * 8 * (best_cost ? 2 : 1);
  s->K4.insert(s->K4.end(), K4, K4 + 16 * (size_t)n);
  s->RT4.insert(s->RT4.end(), RT4, RT4 + 16 * (size_t)n);
  s->n = (int32_t)total;
  drop_points(s);
  return DMI_OK;
}

// One piece of a step: `count` views from view `first`, `offset` pixels into a plane and `elems` pixels long; D's and the alternate
// plane's
struct PieceSpan {
  int64_t first, count;
  size_t offset, elems;
  const double *src;
  double *dst;
};

// The pieces of a step, one after the other: `passes` queues a piece's work from D into the alternate plane around s->events[0 ..
// n_events), `report` the report kernels behind it; the piece of the int32 plane s->aux comes down where out_plane asks for it, and
// the piece is waited for.  Every piece has succeeded: the step ends (end_step).  pass_ms: what the step has timed before its pieces.
template <typename Passes, typename Report>
int run_pieces(dmi_view_set *s, const Pieces &p, rules::Step step, int n_events, int32_t *out_plane, double pass_ms,
               dmi_views_step_report *r, Passes &&passes, Report &&report) {
  double report_ms = 0.0;
  for (int64_t q = 0; q < p.count; ++q) {
    const rules::Piece at = rules::piece_at(s->n, p.per, q);
    const size_t offset = (size_t)at.first * p.plane, elems = (size_t)at.count * p.plane;
    const PieceSpan piece{at.first, at.count, offset, elems, plane_of(s, s->current) + offset, plane_of(s, s->current ^ 1) + offset};
    int rc = passes(piece);
    if (rc != DMI_OK) return rc;
    VS_HIP(s, hipEventRecord(s->report_events[0], s->stream));
    if ((rc = report(piece)) != DMI_OK) return rc;
    VS_HIP(s, hipEventRecord(s->report_events[1], s->stream));
    if (out_plane) VS_HIP(s, hipMemcpyAsync(out_plane + offset, s->aux.ptr, elems * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    if ((rc = end_piece(s, n_events, &pass_ms, &report_ms)) != DMI_OK) return rc;
  }
  if (out_plane) s->d2h_plane_bytes += (uint64_t)s->n * p.plane * sizeof(int32_t);
  return end_step(s, step, pass_ms, report_ms, r);
}

int filter_speckles(dmi_view_set *s, double abs_tolerance, double rel_tolerance, int64_t min_pixels, int32_t *out_size,
                    dmi_views_step_report *r) {
  const std::string entry = "dmi_views_filter_speckles: ";
  if (const int rc = require_set(s, entry)) return rc;
  auto bad = [&](const std::string &what) { return fail(s, DMI_ERR_INVALID_ARGUMENT, entry + what); };
  if (const int rc = require_views(s, entry)) return rc;
  if (min_pixels < 0) return bad("min_pixels >= 0 required");
  if (const char *what = dmi::tolerance_refusal(abs_tolerance, rel_tolerance)) return bad(what);

  const int W = s->W, H = s->H;
  const dmi::SpeckleTuning tuning = dmi::speckle_tuning_from_environment();
  const Pieces p = pieces_of(s, s->n);
  const size_t tiles = (size_t)dmi::speckle_tiles(W, H, p.per, tuning);
  const int rc = begin_step(s);
  if (rc != DMI_OK) return rc;
  VS_HIP(s, grow(s, s->label, (uint64_t)p.per * p.plane * sizeof(uint32_t)));
  VS_HIP(s, grow(s, s->record, (uint64_t)p.per * p.plane * sizeof(uint32_t)));
  VS_HIP(s, grow(s, s->border_down, tiles * sizeof(uint64_t)));
  VS_HIP(s, grow(s, s->border_right, tiles * sizeof(uint64_t)));
  if (out_size) VS_HIP(s, grow(s, s->aux, (uint64_t)p.per * p.plane * sizeof(int32_t)));

  dmi::SpecklePiece piece{};
  return run_pieces(
      s, p, rules::kSpeckles, 5, out_size, 0.0, r,
      [&](const PieceSpan &at) -> int {  // the passes work in place: on a copy of D's piece
        piece = dmi::speckle_piece(at.dst, nullptr, s->label, s->record, s->border_down, s->border_right,
                                   out_size ? s->aux.as<int32_t>() : nullptr, at.count);
        VS_HIP(s, hipMemcpyAsync(piece.depth, at.src, at.elems * 8, hipMemcpyDeviceToDevice, s->stream));
        VS_HIP(s, dmi::run_speckle_piece(piece, 0.0, W, H, abs_tolerance, rel_tolerance, min_pixels, tuning, s->stream, s->events));
        return DMI_OK;
      },
      [&](const PieceSpan &at) -> int {
        VS_HIP(s, dmi::launch_view_set_segment_roots(piece, W, H, min_pixels, counters_of(s), s->compute_units, s->stream));
        VS_HIP(s, dmi::launch_view_set_report(at.src, piece.depth, nullptr, at.elems, counters_of(s), s->compute_units, s->stream));
        return DMI_OK;
      });
}

int fill_holes(dmi_view_set *s, double abs_tolerance, double rel_tolerance, int64_t max_pixels, int32_t *out_size,
               dmi_views_step_report *r) {
  const std::string entry = "dmi_views_fill_holes: ";
  if (const int rc = require_set(s, entry)) return rc;
  auto bad = [&](const std::string &what) { return fail(s, DMI_ERR_INVALID_ARGUMENT, entry + what); };
  if (const int rc = require_views(s, entry)) return rc;
  if (max_pixels < 0) return bad("max_pixels >= 0 required");
  if (const char *what = dmi::tolerance_refusal(abs_tolerance, rel_tolerance)) return bad(what);

  const int W = s->W, H = s->H;
  const Pieces p = pieces_of(s, s->n);
  const size_t tiles = (size_t)dmi::holes_tiles(W, H, p.per);
  const int rc = begin_step(s);
  if (rc != DMI_OK) return rc;
  VS_HIP(s, grow(s, s->label, (uint64_t)p.per * p.plane * sizeof(uint32_t)));
  VS_HIP(s, grow(s, s->record, (uint64_t)p.per * p.plane * sizeof(uint32_t)));
  VS_HIP(s, grow(s, s->rim_lo, (uint64_t)p.per * p.plane * sizeof(uint64_t)));
  VS_HIP(s, grow(s, s->rim_hi, (uint64_t)p.per * p.plane * sizeof(uint64_t)));
  VS_HIP(s, grow(s, s->border_down, tiles * sizeof(uint64_t)));
  VS_HIP(s, grow(s, s->border_right, tiles * sizeof(uint64_t)));
  if (out_size) VS_HIP(s, grow(s, s->aux, (uint64_t)p.per * p.plane * sizeof(int32_t)));

  dmi::HolesPiece piece{};
  return run_pieces(
      s, p, rules::kHoles, 5, out_size, 0.0, r,
      [&](const PieceSpan &at) -> int {  // the output pass writes hole pixels only: into a copy of D's piece
        piece = dmi::holes_piece(at.dst, nullptr, s->label, s->record, s->rim_lo, s->rim_hi, s->border_down, s->border_right,
                                 out_size ? s->aux.as<int32_t>() : nullptr, at.count);
        VS_HIP(s, hipMemcpyAsync(piece.depth, at.src, at.elems * 8, hipMemcpyDeviceToDevice, s->stream));
        VS_HIP(s, dmi::run_holes_piece(piece, 0.0, W, H, abs_tolerance, rel_tolerance, max_pixels, s->stream, s->events));
        return DMI_OK;
      },
      [&](const PieceSpan &at) -> int {
        VS_HIP(s, dmi::launch_view_set_hole_roots(piece, W, H, abs_tolerance, rel_tolerance, max_pixels, counters_of(s), s->compute_units,
                                                   s->stream));
        VS_HIP(s, dmi::launch_view_set_report(at.src, piece.depth, nullptr, at.elems, counters_of(s), s->compute_units, s->stream));
        return DMI_OK;
      });
}

int smooth(dmi_view_set *s, double sigma, double truncate, double abs_tolerance, double rel_tolerance, int32_t iterations,
           int32_t *out_count, dmi_views_step_report *r) {
  const std::string entry = "dmi_views_smooth: ";
  if (const int rc = require_set(s, entry)) return rc;
  auto bad = [&](const std::string &what) { return fail(s, DMI_ERR_INVALID_ARGUMENT, entry + what); };
  if (const int rc = require_views(s, entry)) return rc;
  if (!finite_and_not_negative(sigma)) return bad("sigma must be finite and >= 0");
  if (!(truncate > 0.0 && truncate <= 4.0)) return bad("truncate must lie in (0, 4]");
  int32_t radius = 0;
  double weights[dmi::kDepthSmoothMaxRadius + 1];
  if (dmi::depth_smoothing_weights(sigma, truncate, &radius, weights) != 0)
    return bad("the radius ceil(truncate * sigma) must not exceed " + std::to_string(dmi::kDepthSmoothMaxRadius));
  if (const char *what = dmi::tolerance_refusal(abs_tolerance, rel_tolerance)) return bad(what);
  if (iterations < 1 || iterations > dmi::kDepthSmoothMaxIterations)
    return bad("iterations must lie in [1, " + std::to_string(dmi::kDepthSmoothMaxIterations) + "]");

  const int W = s->W, H = s->H;
  const Pieces p = pieces_of(s, s->n);
  const dmi::SmoothArgs args = dmi::smooth_args(weights, radius, abs_tolerance, rel_tolerance);
  const int rc = begin_step(s);
  if (rc != DMI_OK) return rc;
  if (iterations > 1) VS_HIP(s, grow(s, s->second, (uint64_t)p.per * p.plane * 8));
  VS_HIP(s, grow(s, s->aux, (uint64_t)p.per * p.plane * sizeof(int32_t)));  // the report sums the taps whether asked for or not

  int32_t *const count = s->aux.as<int32_t>();
  return run_pieces(
      s, p, rules::kSmooth, 2, out_count, 0.0, r,
      [&](const PieceSpan &at) -> int {
        // the last iteration writes dst: the iterations start on whichever of the two makes it so.  D is read, never written.
        double *const other = s->second.as<double>();
        const bool odd = iterations % 2 == 1;
        const double *result = nullptr;
        VS_HIP(s, dmi::run_smooth_piece(at.src, nullptr, 0.0, odd ? at.dst : other, odd ? other : at.dst, count, at.count, W, H, args,
                                         iterations, s->stream, s->events, &result));
        if (result != at.dst) return fail(s, DMI_ERR_STATE, entry + "the iterations did not end in the alternate plane");
        return DMI_OK;
      },
      [&](const PieceSpan &at) -> int {
        VS_HIP(s, dmi::launch_view_set_report(at.src, at.dst, count, at.elems, counters_of(s), s->compute_units, s->stream));
        return DMI_OK;
      });
}

// D of every piece into s->flipped, thresholded already, rows flipped to image order (8g's upload pass, device to device)
int flip_planes(dmi_view_set *s, const Pieces &p, double *pass_ms) {
  for (int64_t q = 0; q < p.count; ++q) {
    const rules::Piece at = rules::piece_at(s->n, p.per, q);
    VS_HIP(s, dmi::flip_piece(plane_of(s, s->current) + (size_t)at.first * p.plane, nullptr, 0.0, s->W, s->H, at.first, at.count,
                              s->flipped.as<double>(), s->stream, s->events, pass_ms));
  }
  return DMI_OK;
}

int upload_cameras(dmi_view_set *s) {
  const size_t views = (size_t)s->n;
  VS_HIP(s, grow(s, s->cameras, views * sizeof(dmi::ConsistencyCamera)));
  VS_HIP(s, dmi::upload_cameras(s->cameras, s->K4.data(), s->RT4.data(), views, s->stream));
  return DMI_OK;
}

// What the consistency filter and the point cloud open with, behind begin_step and with a WholeSetScratch standing: the flipped
// planes and the counts grown, then `more` in its order, the cameras up, the counts and what of `more` asks for it zeroed, D flipped
// (its time added to *flip_ms) and, with more than one view, counted (added to *count_ms).
struct Scratch {
  dmi::DeviceBuffer *buffer;
  uint64_t bytes;
  bool zeroed;
};
int flip_and_count(dmi_view_set *s, const Pieces &p, double abs_tolerance, double rel_tolerance, const std::vector<Scratch> &more,
                   double *flip_ms, double *count_ms) {
  const int n = s->n;
  const dmi::ConsistencyTuning tuning = dmi::consistency_tuning_from_environment();
  VS_HIP(s, grow(s, s->flipped, (uint64_t)n * p.plane * 8));
  VS_HIP(s, grow(s, s->counts, (uint64_t)n * p.plane * sizeof(int32_t)));
  for (const Scratch &m : more) VS_HIP(s, grow(s, *m.buffer, m.bytes));
  int rc = upload_cameras(s);
  if (rc != DMI_OK) return rc;
  VS_HIP(s, hipMemsetAsync(s->counts.ptr, 0, (size_t)n * p.plane * sizeof(int32_t), s->stream));
  for (const Scratch &m : more)
    if (m.zeroed) VS_HIP(s, hipMemsetAsync(m.buffer->ptr, 0, (size_t)m.bytes, s->stream));
  if ((rc = flip_planes(s, p, flip_ms)) != DMI_OK) return rc;
  if (n > 1) {
    VS_HIP(s, dmi::run_consistency_count(s->flipped.as<double>(), s->cameras.as<dmi::ConsistencyCamera>(), n, s->W, s->H, abs_tolerance,
                                          rel_tolerance, tuning, s->counts.as<int32_t>(), nullptr, s->stream, s->events));
    VS_HIP(s, hipStreamSynchronize(s->stream));
    VS_HIP(s, dmi::add_spans(s->events, 1, count_ms));
  }
  return DMI_OK;
}

int filter_consistency(dmi_view_set *s, double abs_tolerance, double rel_tolerance, int32_t min_views, int32_t *out_count,
                       dmi_views_step_report *r) {
  const std::string entry = "dmi_views_filter_consistency: ";
  if (const int rc = require_set(s, entry)) return rc;
  auto bad = [&](const std::string &what) { return fail(s, DMI_ERR_INVALID_ARGUMENT, entry + what); };
  if (const int rc = require_views(s, entry)) return rc;
  if (min_views < 0) return bad("min_views >= 0 required");
  if (const char *what = dmi::tolerance_refusal(abs_tolerance, rel_tolerance)) return bad(what);
  if (const int32_t m = dmi::first_view_with_other_k(s->K4.data(), s->n); m >= 0) return bad(dmi::other_k_message(m));

  const int W = s->W, H = s->H;
  const Pieces p = pieces_of(s, s->n);
  int rc = begin_step(s);
  if (rc != DMI_OK) return rc;
  WholeSetScratch scratch{s};
  std::vector<Scratch> more;
  if (out_count) more.push_back({&s->aux, (uint64_t)p.per * p.plane * sizeof(int32_t), false});
  double pass_ms = 0.0;
  if ((rc = flip_and_count(s, p, abs_tolerance, rel_tolerance, more, &pass_ms, &pass_ms)) != DMI_OK) return rc;
  return run_pieces(
      s, p, rules::kConsistency, 2, out_count, pass_ms, r,
      [&](const PieceSpan &at) -> int {
        VS_HIP(s, hipEventRecord(s->events[0], s->stream));
        VS_HIP(s, dmi::launch_consistency_finish(s->flipped.as<double>(), s->counts.as<int32_t>(), W, H, at.first, at.count, min_views, at.dst,
                                                  out_count ? s->aux.as<int32_t>() : nullptr, s->stream));
        VS_HIP(s, hipEventRecord(s->events[1], s->stream));
        return DMI_OK;
      },
      [&](const PieceSpan &at) -> int {
        VS_HIP(s, dmi::launch_view_set_report(at.src, at.dst, nullptr, at.elems, counters_of(s), s->compute_units, s->stream));
        return DMI_OK;
      });
}

int estimate_bounds(dmi_view_set *s, const double *axes9, double trim_fraction, int32_t pixel_step, double lo[3], double hi[3],
                    uint64_t *n_points, double *kernel_ms) {
  const std::string entry = "dmi_views_estimate_bounds: ";
  if (const int rc = require_set(s, entry)) return rc;
  auto bad = [&](const std::string &what) { return fail(s, DMI_ERR_INVALID_ARGUMENT, entry + what); };
  if (!lo) return bad("lo is null");
  if (!hi) return bad("hi is null");
  if (!n_points) return bad("n_points is null");
  if (const int rc = require_views(s, entry)) return rc;
  if ((uint64_t)s->n * (uint64_t)s->W * (uint64_t)s->H >= (uint64_t(1) << 53)) return bad("n * W * H must stay below 2^53");
  if (!(trim_fraction >= 0.0 && trim_fraction <= 0.5)) return bad("trim_fraction must lie in [0, 0.5]");  // false for NaN
  if (pixel_step < 1) return bad("pixel_step >= 1 required");
  dmi::BoundsAxes axes;
  if (!dmi::bounds_axes(axes9, &axes)) return bad("axes9 holds a value that is not finite");
  if (const int32_t m = dmi::first_view_with_other_k(s->K4.data(), s->n); m >= 0) return bad(dmi::other_k_message(m));

  const int n = s->n;
  const dmi::BoundsTuning tuning = dmi::bounds_tuning_from_environment();
  const Pieces p = pieces_of(s, n);
  constexpr size_t kHistBytes = sizeof(unsigned long long) * dmi::bounds_rules::kTargets * dmi::bounds_rules::kBins;
  VS_HIP(s, hipSetDevice(s->device));
  WholeSetScratch scratch{s};
  VS_HIP(s, grow(s, s->flipped, (uint64_t)n * p.plane * 8));
  VS_HIP(s, grow(s, s->state, sizeof(dmi::BoundsState)));
  VS_HIP(s, grow(s, s->hist, kHistBytes));
  int rc = upload_cameras(s);
  if (rc != DMI_OK) return rc;
  VS_HIP(s, hipMemsetAsync(s->state.ptr, 0, sizeof(dmi::BoundsState), s->stream));
  VS_HIP(s, hipMemsetAsync(s->hist.ptr, 0, kHistBytes, s->stream));
  double pass_ms = 0.0;
  if ((rc = flip_planes(s, p, &pass_ms)) != DMI_OK) return rc;
  dmi::BoundsState result;
  VS_HIP(s, dmi::run_bounds_select(s->flipped.as<double>(), s->cameras.as<dmi::ConsistencyCamera>(), n, s->W, s->H, pixel_step, axes,
                                    trim_fraction, s->state.as<dmi::BoundsState>(), s->hist.as<unsigned long long>(), s->compute_units,
                                    tuning, s->stream, s->events, &result));
  VS_HIP(s, dmi::add_spans(s->events, 1, &pass_ms));
  for (int a = 0; a < 3; ++a) {
    lo[a] = result.result[2 * a];
    hi[a] = result.result[2 * a + 1];
  }
  *n_points = result.n;
  if (kernel_ms) *kernel_ms = pass_ms;
  s->steps += 1;
  return DMI_OK;
}

int download(dmi_view_set *s, int32_t first, int32_t count, double *out_depth) {
  const std::string entry = "dmi_views_download: ";
  if (const int rc = require_set(s, entry)) return rc;
  auto bad = [&](const std::string &what) { return fail(s, DMI_ERR_INVALID_ARGUMENT, entry + what); };
  if (!out_depth) return bad("out_depth is null");
  if (const int rc = require_views(s, entry)) return rc;
  if (first < 0 || count < 1 || (int64_t)first + count > s->n) return bad("first and count must name views of the set");
  const size_t plane = (size_t)s->W * (size_t)s->H;
  VS_HIP(s, hipSetDevice(s->device));
  VS_HIP(s, hipMemcpyAsync(out_depth, plane_of(s, s->current) + (size_t)first * plane, (size_t)count * plane * 8, hipMemcpyDeviceToHost,
                            s->stream));
  VS_HIP(s, hipStreamSynchronize(s->stream));
  s->d2h_plane_bytes += (uint64_t)count * plane * 8;
  return DMI_OK;
}

int build_points(dmi_view_set *s, double abs_tolerance, double rel_tolerance, double normal_abs_tolerance, double normal_rel_tolerance,
                 int32_t min_views, int32_t pixel_step, int32_t dedupe, uint64_t *n_points, dmi_views_points_report *r) {
  namespace pr = dmi::points_rules;
  const std::string entry = "dmi_views_build_points: ";
  if (const int rc = require_set(s, entry)) return rc;
  auto bad = [&](const std::string &what) { return fail(s, DMI_ERR_INVALID_ARGUMENT, entry + what); };
  if (!n_points) return bad("n_points is null");
  if (const char *what = dmi::tolerance_refusal(abs_tolerance, rel_tolerance)) return bad(what);
  if (!finite_and_not_negative(normal_abs_tolerance)) return bad("normal_abs_tolerance must be finite and >= 0");
  if (!finite_and_not_negative(normal_rel_tolerance)) return bad("normal_rel_tolerance must be finite and >= 0");
  if (min_views < 0) return bad("min_views >= 0 required");
  if (pixel_step < 1) return bad("pixel_step >= 1 required");
  if (dedupe != 0 && dedupe != 1) return bad("dedupe must be 0 or 1");
  if (const int rc = require_views(s, entry)) return rc;
  if (!pr::blocks_fit_one_launch(s->n, s->W, s->H)) return bad("n * ceil(W * H / 256) must stay below 2^31");
  if (const int32_t m = dmi::first_view_with_other_k(s->K4.data(), s->n); m >= 0) return bad(dmi::other_k_message(m));

  const int W = s->W, H = s->H, n = s->n;
  const Pieces p = pieces_of(s, n);
  const int64_t blocks = pr::total_blocks(n, W, H);
  const dmi::PointsParams params{W, H, min_views, pixel_step, dedupe, abs_tolerance, rel_tolerance, normal_abs_tolerance,
                                 normal_rel_tolerance};
  int rc = begin_step(s);
  if (rc != DMI_OK) return rc;
  WholeSetScratch scratch{s};
  double pass_ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  rc = flip_and_count(s, p, abs_tolerance, rel_tolerance,
                      {{&s->flags, (uint64_t)n * p.plane, true},
                       {&s->block_counts, (uint64_t)blocks * sizeof(uint32_t), false},
                       {&s->block_offsets, ((uint64_t)blocks + 1) * sizeof(uint64_t), false}},  // the total stands behind the offsets
                      &pass_ms[0], &pass_ms[1]);
  if (rc != DMI_OK) return rc;
  uint64_t *const offsets = s->block_offsets.as<uint64_t>();
  VS_HIP(s, hipEventRecord(s->events[0], s->stream));
  VS_HIP(s, dmi::launch_points_flags(s->flipped.as<double>(), s->counts.as<int32_t>(), s->cameras.as<dmi::ConsistencyCamera>(), n, params,
                                      s->flags.as<uint8_t>(), s->stream));
  VS_HIP(s, hipEventRecord(s->events[1], s->stream));
  VS_HIP(s, dmi::launch_points_block_counts(s->flags.as<uint8_t>(), n, W, H, s->block_counts.as<uint32_t>(), s->stream));
  VS_HIP(s, dmi::launch_points_scan(s->block_counts.as<uint32_t>(), blocks, offsets, offsets + blocks, counters_of(s), s->stream));
  VS_HIP(s, hipEventRecord(s->events[2], s->stream));
  uint64_t total = 0;
  VS_HIP(s, hipMemcpyAsync(&total, offsets + blocks, sizeof(total), hipMemcpyDeviceToHost, s->stream));
  VS_HIP(s, hipStreamSynchronize(s->stream));

  // the arrays, at exactly the size needed; the points of an earlier build stay until these are complete
  pr::Layout layout;
  if (!pr::layout_of(total, &layout)) return fail(s, DMI_ERR_OUT_OF_MEMORY, entry + "the points do not fit 64 bits of bytes");
  dmi::DeviceBuffer fresh;
  struct Guard {
    dmi_view_set *s;
    dmi::DeviceBuffer *b;
    ~Guard() { dmi::free_buffers({b}, s->device_bytes); }  // (empty once the buffer has become the set's)
  } guard{s, &fresh};
  if (total) VS_HIP(s, grow(s, fresh, layout.bytes));
  VS_HIP(s, hipEventRecord(s->events[3], s->stream));
  if (total) {  // (the block counts have been scanned: their memory takes the blocks' normals)
    VS_HIP(s, dmi::launch_points_scatter(s->flipped.as<double>(), s->counts.as<int32_t>(), s->cameras.as<dmi::ConsistencyCamera>(),
                                          s->flags.as<uint8_t>(), n, params, offsets, layout, fresh.as<unsigned char>(),
                                          s->block_counts.as<uint32_t>(), s->stream));
    VS_HIP(s, dmi::launch_points_sum_normals(s->block_counts.as<uint32_t>(), blocks, counters_of(s), s->stream));
  }
  VS_HIP(s, hipEventRecord(s->events[4], s->stream));
  unsigned long long c[dmi::kPtCounters];
  VS_HIP(s, hipMemcpyAsync(c, s->counters.ptr, sizeof(c), hipMemcpyDeviceToHost, s->stream));
  VS_HIP(s, hipStreamSynchronize(s->stream));
  VS_HIP(s, dmi::add_spans(s->events, 2, &pass_ms[2]));
  VS_HIP(s, dmi::add_spans(s->events + 3, 1, &pass_ms[4]));

  drop_points(s);
  std::swap(s->points, fresh);
  s->n_points = total;
  s->points_current = true;
  s->steps += 1;
  double kernel_ms = 0.0;
  for (int e = 0; e < 5; ++e) kernel_ms += (s->points_pass_ms[e] = pass_ms[e]);
  *n_points = total;
  if (r) {
    r->valid = c[dmi::kPtValid];
    r->candidates = c[dmi::kPtCandidates];
    r->owned = c[dmi::kPtOwned];
    r->points = total;
    r->with_normal = c[dmi::kPtWithNormal];
    r->kernel_ms = kernel_ms;
  }
  return DMI_OK;
}

int download_points(dmi_view_set *s, uint64_t first, uint64_t count, double *xyz, float *normal, int32_t *view, int32_t *pixel,
                    int32_t *n_views) {
  namespace pr = dmi::points_rules;
  const std::string entry = "dmi_views_download_points: ";
  if (const int rc = require_set(s, entry)) return rc;
  if (!s->points_current) return fail(s, DMI_ERR_STATE, entry + "the set holds no points: dmi_views_build_points comes first");
  if (first > s->n_points || count > s->n_points - first)
    return fail(s, DMI_ERR_INVALID_ARGUMENT, entry + "first + count must not exceed the number of points");
  if (count == 0) return DMI_OK;
  pr::Layout layout;
  (void)pr::layout_of(s->n_points, &layout);  // (it fitted when the points were built)
  const unsigned char *const base = s->points.as<unsigned char>();
  VS_HIP(s, hipSetDevice(s->device));
  auto copy = [&](void *dst, uint64_t array, uint64_t stride) {
    return dst ? hipMemcpyAsync(dst, base + pr::entry_offset(array, first, stride), (size_t)(count * stride), hipMemcpyDeviceToHost,
                                s->stream)
               : hipSuccess;
  };
  VS_HIP(s, copy(xyz, layout.xyz, 24));
  VS_HIP(s, copy(normal, layout.normal, 12));
  VS_HIP(s, copy(view, layout.view, 4));
  VS_HIP(s, copy(pixel, layout.pixel, 4));
  VS_HIP(s, copy(n_views, layout.count, 4));
  VS_HIP(s, hipStreamSynchronize(s->stream));
  return DMI_OK;
}

// the set's cloud replaced by its thinned one: dmi::run_thin_points (dmi_capi_points_thin.hip) on the arrays of s->points
int thin_points(dmi_view_set *s, double cell_size, int32_t min_points, uint64_t *n_points, dmi_points_thin_report *r) {
  namespace pr = dmi::points_rules;
  const std::string entry = "dmi_views_thin_points";
  if (const int rc = require_set(s, entry + ": ")) return rc;
  auto bad = [&](const std::string &what) { return fail(s, DMI_ERR_INVALID_ARGUMENT, entry + ": " + what); };
  if (!n_points) return bad("n_points is null");
  if (!(cell_size > 0.0) || cell_size - cell_size != 0.0) return bad("cell_size is not a finite number > 0");
  if (min_points < 1) return bad("min_points >= 1 required");
  if (!s->points_current) return fail(s, DMI_ERR_STATE, entry + ": the set holds no points: dmi_views_build_points comes first");
  if (s->points_thinned)
    return fail(s, DMI_ERR_STATE, entry + ": the cloud is thinned already (a centroid of centroids is not the centroid): build again");
  if (s->n_points > dmi::thin_rules::kMaxPoints) return bad("the cloud must hold fewer than 2^32 points");

  VS_HIP(s, hipSetDevice(s->device));
  dmi::ThinOutcome outcome;
  if (s->n_points) {
    pr::Layout in;
    (void)pr::layout_of(s->n_points, &in);  // (it fitted when the points were built)
    const unsigned char *const base = s->points.as<unsigned char>();
    dmi::ThinCloud cloud{};
    cloud.xyz = reinterpret_cast<const double *>(base + in.xyz);
    cloud.normal = reinterpret_cast<const float *>(base + in.normal);
    cloud.view = reinterpret_cast<const int32_t *>(base + in.view);
    cloud.pixel = reinterpret_cast<const int32_t *>(base + in.pixel);
    cloud.count = reinterpret_cast<const int32_t *>(base + in.count);
    cloud.n = s->n_points;
    std::string message;
    const int rc = dmi::run_thin_points(entry, cloud, cell_size, min_points, s->thin_wave_cell_points, s->stream, s->device_bytes,
                                        &outcome, &message);
    if (rc != DMI_OK) return fail(s, rc, message);  // (nothing of the call is left; the cloud is as it was)
  }
  dmi::free_buffers({&s->points, &s->plane_rms}, s->device_bytes);  // (a fit's plane_rms went with the old cloud)
  s->points_fitted = false;
  s->points = outcome.result;
  s->n_points = outcome.n_out;
  s->points_thinned = true;
  s->points_filtered = false;  // (the counts went with the old cloud)
  s->steps += 1;
  for (int e = 0; e < 5; ++e) s->thin_pass_ms[e] = outcome.pass_ms[e];
  *n_points = outcome.n_out;
  if (r) *r = outcome.report;
  return DMI_OK;
}

int download_point_members(dmi_view_set *s, uint64_t first, uint64_t count, uint32_t *out) {
  const std::string entry = "dmi_views_download_point_members: ";
  if (const int rc = require_set(s, entry)) return rc;
  if (!s->points_current) return fail(s, DMI_ERR_STATE, entry + "the set holds no points: dmi_views_build_points comes first");
  if (first > s->n_points || count > s->n_points - first)
    return fail(s, DMI_ERR_INVALID_ARGUMENT, entry + "first + count must not exceed the number of points");
  if (count == 0) return DMI_OK;
  if (!out) return fail(s, DMI_ERR_INVALID_ARGUMENT, entry + "out is null");
  if (!s->points_thinned) {  // every point of a built cloud is one pixel
    std::fill(out, out + count, 1u);
    return DMI_OK;
  }
  dmi::thin_rules::Layout layout;
  (void)dmi::thin_rules::layout_of(s->n_points, &layout);
  VS_HIP(s, hipSetDevice(s->device));
  VS_HIP(s, hipMemcpyAsync(out, s->points.as<unsigned char>() + layout.members + first * 4, (size_t)(count * 4), hipMemcpyDeviceToHost,
                            s->stream));
  VS_HIP(s, hipStreamSynchronize(s->stream));
  return DMI_OK;
}

// the set's cloud, built or thinned, replaced by its points with at least min_neighbors neighbours within radius:
// dmi::run_radius_points (dmi_capi_points_radius.hip) on the arrays of s->points
int filter_points_radius(dmi_view_set *s, double radius, int32_t min_neighbors, uint64_t *n_points, dmi_points_radius_report *r) {
  const std::string entry = "dmi_views_filter_points_radius";
  if (const int rc = require_set(s, entry + ": ")) return rc;
  auto bad = [&](const std::string &what) { return fail(s, DMI_ERR_INVALID_ARGUMENT, entry + ": " + what); };
  if (!n_points) return bad("n_points is null");
  if (const char *what = dmi::radius_refusal(radius, min_neighbors)) return bad(what);
  if (!s->points_current) return fail(s, DMI_ERR_STATE, entry + ": the set holds no points: dmi_views_build_points comes first");
  if (s->n_points > dmi::radius_rules::kMaxPoints) return bad("the cloud must hold fewer than 2^32 points");

  VS_HIP(s, hipSetDevice(s->device));
  dmi::RadiusOutcome outcome;
  if (s->n_points) {
    dmi::thin_rules::Layout in;
    (void)dmi::thin_rules::layout_of(s->n_points, &in);  // (it fitted when the points were made; the first five arrays are the build's)
    const unsigned char *const base = s->points.as<unsigned char>();
    dmi::RadiusCloud cloud{};
    cloud.xyz = reinterpret_cast<const double *>(base + in.xyz);
    cloud.normal = reinterpret_cast<const float *>(base + in.normal);
    cloud.view = reinterpret_cast<const int32_t *>(base + in.view);
    cloud.pixel = reinterpret_cast<const int32_t *>(base + in.pixel);
    cloud.count = reinterpret_cast<const int32_t *>(base + in.count);
    cloud.members = s->points_thinned ? reinterpret_cast<const uint32_t *>(base + in.members) : nullptr;
    cloud.n = s->n_points;
    std::string message;
    const int rc = dmi::run_radius_points(entry, cloud, radius, min_neighbors, s->radius_group_points, s->points_thinned ? 52 : 48,
                                          s->stream, s->device_bytes, &outcome, &message);
    if (rc != DMI_OK) return fail(s, rc, message);  // (nothing of the call is left; the cloud is as it was)
  }
  dmi::free_buffers({&s->points, &s->plane_rms}, s->device_bytes);  // (a fit's plane_rms went with the old cloud)
  s->points_fitted = false;
  s->points = outcome.result;
  s->n_points = outcome.n_kept;
  s->points_filtered = true;
  s->steps += 1;
  for (int e = 0; e < 7; ++e) s->radius_pass_ms[e] = outcome.pass_ms[e];
  *n_points = outcome.n_kept;
  if (r) *r = outcome.report;
  return DMI_OK;
}

int download_point_neighbors(dmi_view_set *s, uint64_t first, uint64_t count, uint32_t *out) {
  const std::string entry = "dmi_views_download_point_neighbors: ";
  if (const int rc = require_set(s, entry)) return rc;
  if (!s->points_current || !s->points_filtered)
    return fail(s, DMI_ERR_STATE, entry + "the current cloud did not come out of dmi_views_filter_points_radius");
  if (first > s->n_points || count > s->n_points - first)
    return fail(s, DMI_ERR_INVALID_ARGUMENT, entry + "first + count must not exceed the number of points");
  if (count == 0) return DMI_OK;
  if (!out) return fail(s, DMI_ERR_INVALID_ARGUMENT, entry + "out is null");
  uint64_t neighbors_offset = 0, bytes = 0;
  (void)dmi::radius_rules::filtered_bytes(s->n_points, s->points_thinned ? 52 : 48, &neighbors_offset, &bytes);
  VS_HIP(s, hipSetDevice(s->device));
  VS_HIP(s, hipMemcpyAsync(out, s->points.as<unsigned char>() + neighbors_offset + first * 4, (size_t)(count * 4), hipMemcpyDeviceToHost,
                            s->stream));
  VS_HIP(s, hipStreamSynchronize(s->stream));
  return DMI_OK;
}

// the set's cloud -- built, thinned or filtered -- replaced by one of the same layout whose points lie on the planes fitted to their
// balls and carry those planes' normals: dmi::run_plane_fit_points (dmi_capi_points_planes.hip) from the arrays of s->points into
// a copy of them
int fit_point_planes(dmi_view_set *s, double radius, int32_t min_neighbors, int32_t flags, dmi_points_planes_report *r) {
  const std::string entry = "dmi_views_fit_point_planes";
  if (const int rc = require_set(s, entry + ": ")) return rc;
  auto bad = [&](const std::string &what) { return fail(s, DMI_ERR_INVALID_ARGUMENT, entry + ": " + what); };
  if (const char *what = dmi::plane_fit_refusal(radius, min_neighbors, flags)) return bad(what);
  if (!s->points_current) return fail(s, DMI_ERR_STATE, entry + ": the set holds no points: dmi_views_build_points comes first");
  if (s->n_points > dmi::radius_rules::kMaxPoints) return bad("the cloud must hold fewer than 2^32 points");

  VS_HIP(s, hipSetDevice(s->device));
  dmi::PlaneFitOutcome outcome;
  dmi::DeviceBuffer fresh;
  struct Guard {
    dmi_view_set *s;
    dmi::DeviceBuffer *b;
    ~Guard() { dmi::free_buffers({b}, s->device_bytes); }  // (empty once the buffer has become the set's)
  } guard{s, &fresh};
  if (s->n_points) {
    dmi::thin_rules::Layout in;
    (void)dmi::thin_rules::layout_of(s->n_points, &in);  // (it fitted when the points were made; the first five arrays are the build's)
    uint64_t neighbors_offset = 0, bytes = (s->points_thinned ? 52 : 48) * s->n_points;
    if (s->points_filtered) (void)dmi::radius_rules::filtered_bytes(s->n_points, s->points_thinned ? 52 : 48, &neighbors_offset, &bytes);
    const unsigned char *const base = s->points.as<unsigned char>();
    VS_HIP(s, grow(s, fresh, bytes));
    VS_HIP(s, hipMemcpyAsync(fresh.ptr, base, (size_t)bytes, hipMemcpyDeviceToDevice, s->stream));  // every array keeps its bits ...
    unsigned char *const out = fresh.as<unsigned char>();
    std::string message;
    const int rc = dmi::run_plane_fit_points(entry, reinterpret_cast<const double *>(base + in.xyz),
                                             reinterpret_cast<const float *>(base + in.normal), s->n_points, radius, min_neighbors, flags,
                                             s->radius_group_points, reinterpret_cast<double *>(out + in.xyz),  // ... but the fitted points'
                                             reinterpret_cast<float *>(out + in.normal), s->stream, s->device_bytes, &outcome, &message);
    if (rc != DMI_OK) return fail(s, rc, message);  // (nothing of the call is left; the cloud is as it was)
    dmi::free_buffers({&outcome.neighbors}, s->device_bytes);  // (the report has their sums; a filtered cloud keeps the filter's counts)
    std::swap(s->points, fresh);  // (the guard frees the old cloud)
  }
  dmi::free_buffers({&s->plane_rms}, s->device_bytes);
  s->plane_rms = outcome.plane_rms;
  s->points_fitted = true;
  s->steps += 1;
  for (int e = 0; e < 6; ++e) s->plane_fit_pass_ms[e] = outcome.pass_ms[e];
  if (r) *r = outcome.report;
  return DMI_OK;
}

int download_point_plane_rms(dmi_view_set *s, uint64_t first, uint64_t count, float *out) {
  const std::string entry = "dmi_views_download_point_plane_rms: ";
  if (const int rc = require_set(s, entry)) return rc;
  if (!s->points_current || !s->points_fitted)
    return fail(s, DMI_ERR_STATE, entry + "the current cloud did not come out of dmi_views_fit_point_planes");
  if (first > s->n_points || count > s->n_points - first)
    return fail(s, DMI_ERR_INVALID_ARGUMENT, entry + "first + count must not exceed the number of points");
  if (count == 0) return DMI_OK;
  if (!out) return fail(s, DMI_ERR_INVALID_ARGUMENT, entry + "out is null");
  VS_HIP(s, hipSetDevice(s->device));
  VS_HIP(s, hipMemcpyAsync(out, s->plane_rms.as<float>() + first, (size_t)(count * 4), hipMemcpyDeviceToHost, s->stream));
  VS_HIP(s, hipStreamSynchronize(s->stream));
  return DMI_OK;
}

}  // namespace

extern "C" {

int dmi_views_create(int32_t device, int32_t W, int32_t H, dmi_view_set **out) {
  return guarded(nullptr, "dmi_views_create", [&]() -> int { return create(device, W, H, out); });
}

void dmi_views_destroy(dmi_view_set *s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  dmi::free_buffers({&s->plane[0], &s->plane[1], &s->stage_depth, &s->stage_cost, &s->label, &s->record, &s->rim_lo, &s->rim_hi,
                     &s->border_down, &s->border_right, &s->second, &s->aux, &s->flipped, &s->counts, &s->cameras, &s->state, &s->hist,
                     &s->flags, &s->block_counts, &s->block_offsets, &s->points, &s->plane_rms, &s->counters});
  dmi::destroy_events(s->events);
  dmi::destroy_events(s->report_events);
  if (s->handed_over) (void)hipEventDestroy(s->handed_over);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  (void)hipGetLastError();
  delete s;
}

const char *dmi_views_last_error(const dmi_view_set *s) { return s ? s->err.c_str() : dmi::g_create_error.c_str(); }

int dmi_views_add(dmi_view_set *s, const double *depth, const double *best_cost, double threshold, const double *K4, const double *RT4,
                  int32_t n) {
  return guarded(s, "dmi_views_add", [&]() -> int { return add(s, depth, best_cost, threshold, K4, RT4, n); });
}

int dmi_views_clear(dmi_view_set *s) {
  return guarded(s, "dmi_views_clear", [&]() -> int {
    if (const int rc = require_set(s, "dmi_views_clear: ")) return rc;
    drop_points(s);
    s->n = 0;
    s->K4.clear();
    s->RT4.clear();
    return DMI_OK;
  });
}

int dmi_views_get_info(dmi_view_set *s, dmi_views_info *out) {
  return guarded(s, "dmi_views_get_info", [&]() -> int {
    if (const int rc = require_set(s, "dmi_views_get_info: ")) return rc;
    if (!out) return fail(s, DMI_ERR_INVALID_ARGUMENT, "dmi_views_get_info: out is null");
    out->n = s->n;
    out->W = s->W;
    out->H = s->H;
    out->device = s->device;
    out->device_bytes = s->device_bytes;
    out->steps = s->steps;
    out->h2d_plane_bytes = s->h2d_plane_bytes;
    out->d2h_plane_bytes = s->d2h_plane_bytes;
    out->last_report_kernel_ms = s->last_report_kernel_ms;
    return DMI_OK;
  });
}

size_t dmi_sizeof_views_info(void) { return sizeof(dmi_views_info); }

int dmi_views_set_piece_bytes(dmi_view_set *s, uint64_t bytes) {
  return guarded(s, "dmi_views_set_piece_bytes", [&]() -> int {
    if (const int rc = require_set(s, "dmi_views_set_piece_bytes: ")) return rc;
    if (bytes == 0) return fail(s, DMI_ERR_INVALID_ARGUMENT, "dmi_views_set_piece_bytes: bytes >= 1 required");
    s->piece_bytes = bytes;
    return DMI_OK;
  });
}

int dmi_views_filter_speckles(dmi_view_set *s, double abs_tolerance, double rel_tolerance, int64_t min_pixels, int32_t *out_size,
                              dmi_views_step_report *r) {
  return guarded(s, "dmi_views_filter_speckles",
                 [&]() -> int { return filter_speckles(s, abs_tolerance, rel_tolerance, min_pixels, out_size, r); });
}

int dmi_views_fill_holes(dmi_view_set *s, double abs_tolerance, double rel_tolerance, int64_t max_pixels, int32_t *out_size,
                         dmi_views_step_report *r) {
  return guarded(s, "dmi_views_fill_holes", [&]() -> int { return fill_holes(s, abs_tolerance, rel_tolerance, max_pixels, out_size, r); });
}

int dmi_views_smooth(dmi_view_set *s, double sigma, double truncate, double abs_tolerance, double rel_tolerance, int32_t iterations,
                     int32_t *out_count, dmi_views_step_report *r) {
  return guarded(s, "dmi_views_smooth",
                 [&]() -> int { return smooth(s, sigma, truncate, abs_tolerance, rel_tolerance, iterations, out_count, r); });
}

int dmi_views_filter_consistency(dmi_view_set *s, double abs_tolerance, double rel_tolerance, int32_t min_views, int32_t *out_count,
                                 dmi_views_step_report *r) {
  return guarded(s, "dmi_views_filter_consistency",
                 [&]() -> int { return filter_consistency(s, abs_tolerance, rel_tolerance, min_views, out_count, r); });
}

int dmi_views_estimate_bounds(dmi_view_set *s, const double *axes9, double trim_fraction, int32_t pixel_step, double lo[3], double hi[3],
                              uint64_t *n_points, double *kernel_ms) {
  return guarded(s, "dmi_views_estimate_bounds",
                 [&]() -> int { return estimate_bounds(s, axes9, trim_fraction, pixel_step, lo, hi, n_points, kernel_ms); });
}

int dmi_views_download(dmi_view_set *s, int32_t first, int32_t count, double *out_depth) {
  return guarded(s, "dmi_views_download", [&]() -> int { return download(s, first, count, out_depth); });
}

int dmi_views_build_points(dmi_view_set *s, double abs_tolerance, double rel_tolerance, double normal_abs_tolerance,
                           double normal_rel_tolerance, int32_t min_views, int32_t pixel_step, int32_t dedupe, uint64_t *n_points,
                           dmi_views_points_report *r) {
  return guarded(s, "dmi_views_build_points", [&]() -> int {
    return build_points(s, abs_tolerance, rel_tolerance, normal_abs_tolerance, normal_rel_tolerance, min_views, pixel_step, dedupe,
                        n_points, r);
  });
}

int dmi_views_download_points(dmi_view_set *s, uint64_t first, uint64_t count, double *xyz, float *normal, int32_t *view, int32_t *pixel,
                              int32_t *n_views) {
  return guarded(s, "dmi_views_download_points",
                 [&]() -> int { return download_points(s, first, count, xyz, normal, view, pixel, n_views); });
}

int dmi_views_get_points_pass_ms(dmi_view_set *s, double out_ms[5]) {
  return guarded(s, "dmi_views_get_points_pass_ms", [&]() -> int {
    if (const int rc = require_set(s, "dmi_views_get_points_pass_ms: ")) return rc;
    if (!out_ms) return fail(s, DMI_ERR_INVALID_ARGUMENT, "dmi_views_get_points_pass_ms: out_ms is null");
    if (!s->points_current) return fail(s, DMI_ERR_STATE, "dmi_views_get_points_pass_ms: the set holds no points");
    for (int e = 0; e < 5; ++e) out_ms[e] = s->points_pass_ms[e];
    return DMI_OK;
  });
}

int dmi_views_thin_points(dmi_view_set *s, double cell_size, int32_t min_points, uint64_t *n_points, dmi_points_thin_report *r) {
  return guarded(s, "dmi_views_thin_points", [&]() -> int { return thin_points(s, cell_size, min_points, n_points, r); });
}

int dmi_views_download_point_members(dmi_view_set *s, uint64_t first, uint64_t count, uint32_t *out) {
  return guarded(s, "dmi_views_download_point_members", [&]() -> int { return download_point_members(s, first, count, out); });
}

int dmi_views_get_thin_pass_ms(dmi_view_set *s, double out_ms[5]) {
  return guarded(s, "dmi_views_get_thin_pass_ms", [&]() -> int {
    if (const int rc = require_set(s, "dmi_views_get_thin_pass_ms: ")) return rc;
    if (!out_ms) return fail(s, DMI_ERR_INVALID_ARGUMENT, "dmi_views_get_thin_pass_ms: out_ms is null");
    if (!s->points_current || !s->points_thinned)
      return fail(s, DMI_ERR_STATE, "dmi_views_get_thin_pass_ms: the set holds no thinned cloud");
    for (int e = 0; e < 5; ++e) out_ms[e] = s->thin_pass_ms[e];
    return DMI_OK;
  });
}

int dmi_views_set_thin_wave_cell_points(dmi_view_set *s, int32_t k) {
  return guarded(s, "dmi_views_set_thin_wave_cell_points", [&]() -> int {
    if (const int rc = require_set(s, "dmi_views_set_thin_wave_cell_points: ")) return rc;
    if (k < 1) return fail(s, DMI_ERR_INVALID_ARGUMENT, "dmi_views_set_thin_wave_cell_points: k >= 1 required");
    s->thin_wave_cell_points = (uint32_t)k;
    return DMI_OK;
  });
}

int dmi_views_filter_points_radius(dmi_view_set *s, double radius, int32_t min_neighbors, uint64_t *n_points, dmi_points_radius_report *r) {
  return guarded(s, "dmi_views_filter_points_radius", [&]() -> int { return filter_points_radius(s, radius, min_neighbors, n_points, r); });
}

int dmi_views_download_point_neighbors(dmi_view_set *s, uint64_t first, uint64_t count, uint32_t *out) {
  return guarded(s, "dmi_views_download_point_neighbors", [&]() -> int { return download_point_neighbors(s, first, count, out); });
}

int dmi_views_get_radius_pass_ms(dmi_view_set *s, double out_ms[7]) {
  return guarded(s, "dmi_views_get_radius_pass_ms", [&]() -> int {
    if (const int rc = require_set(s, "dmi_views_get_radius_pass_ms: ")) return rc;
    if (!out_ms) return fail(s, DMI_ERR_INVALID_ARGUMENT, "dmi_views_get_radius_pass_ms: out_ms is null");
    if (!s->points_current || !s->points_filtered)
      return fail(s, DMI_ERR_STATE, "dmi_views_get_radius_pass_ms: the current cloud did not come out of the radius filter");
    for (int e = 0; e < 7; ++e) out_ms[e] = s->radius_pass_ms[e];
    return DMI_OK;
  });
}

int dmi_views_fit_point_planes(dmi_view_set *s, double radius, int32_t min_neighbors, int32_t flags, dmi_points_planes_report *r) {
  return guarded(s, "dmi_views_fit_point_planes", [&]() -> int { return fit_point_planes(s, radius, min_neighbors, flags, r); });
}

int dmi_views_download_point_plane_rms(dmi_view_set *s, uint64_t first, uint64_t count, float *out) {
  return guarded(s, "dmi_views_download_point_plane_rms", [&]() -> int { return download_point_plane_rms(s, first, count, out); });
}

int dmi_views_get_plane_fit_pass_ms(dmi_view_set *s, double out_ms[6]) {
  return guarded(s, "dmi_views_get_plane_fit_pass_ms", [&]() -> int {
    if (const int rc = require_set(s, "dmi_views_get_plane_fit_pass_ms: ")) return rc;
    if (!out_ms) return fail(s, DMI_ERR_INVALID_ARGUMENT, "dmi_views_get_plane_fit_pass_ms: out_ms is null");
    if (!s->points_current || !s->points_fitted)
      return fail(s, DMI_ERR_STATE, "dmi_views_get_plane_fit_pass_ms: the current cloud did not come out of the plane fit");
    for (int e = 0; e < 6; ++e) out_ms[e] = s->plane_fit_pass_ms[e];
    return DMI_OK;
  });
}

int dmi_views_set_radius_group_points(dmi_view_set *s, int32_t k) {
  return guarded(s, "dmi_views_set_radius_group_points", [&]() -> int {
    if (const int rc = require_set(s, "dmi_views_set_radius_group_points: ")) return rc;
    if (k < 1 || k > (int32_t)dmi::radius_rules::kMaxGroupPoints)
      return fail(s, DMI_ERR_INVALID_ARGUMENT, "dmi_views_set_radius_group_points: k must lie in [1, 64]");
    s->radius_group_points = (uint32_t)k;
    return DMI_OK;
  });
}

}  // extern "C"
