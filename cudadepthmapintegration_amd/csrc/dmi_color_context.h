// dmi_color_context.h -- the context behind the dmi_color_* C ABI of include/dmi.h (dmi_capi_color.hip), in groups: every device
// allocation a dmi::DeviceBuffer (capacity in bytes) grown by one rule, every group with a release().  Private: never installed.
#pragma once
#include "coloration_kernels.h"
#include "dmi_buffer.h"
#include "dmi_context.h"
#include "mesh_depth_render.h"

struct dmi_color_context {
  // the context itself: its device, the stream of every kernel, the last failure's message
  int32_t device = 0;
  hipStream_t stream = nullptr;
  std::string err;

  struct Batch {  // the views of one dmi_color_add_views* call
    dmi::DeviceBuffer rgba;   // n tiled RGBA planes
    dmi::DeviceBuffer depth;  // n tiled f64 depth planes (dmi_color_add_views_with_depth), else empty
    int32_t n = 0;
    void release() { dmi::free_buffers({&rgba, &depth}); }
  };
  struct Views {
    std::vector<Batch> batches;
    std::vector<dmi::ColorView> h_views;
    dmi::DeviceBuffer records;  // h_views on the device
    // the visibility test (dmi_color_set_depth_test): per view its depth plane -- uploaded with its batch, or rendered -- or null
    std::vector<const double *> h_depth_planes;
    dmi::DeviceBuffer depth_planes;
    int32_t W = 0, H = 0;
    bool dirty = false;  // the host tables have changed since they were last copied
    void clear() {       // the views go, the tables' allocations stay
      for (Batch &b : batches) b.release();
      batches.clear();
      h_views.clear();
      h_depth_planes.clear();
      dirty = true;
      W = H = 0;
    }
    void release() { clear(); dmi::free_buffers({&records, &depth_planes}); }
  } views;
  struct Visibility {
    bool depth_test = false;
    double depth_tol = 0.0;
    // the fused form of the test (dmi::color_device_vertices): per view its table in the fusion context, for the call being made
    std::vector<const void *> h_fused_tables;
    dmi::DeviceBuffer fused_tables;
    void release() { dmi::free_buffers({&fused_tables}); }
  } visibility;
  // The per-chunk buffers of a colouring call, grown on demand.  The chunk's magnitudes and margins exist TWICE (and so do the
  // staged form's vertices and outputs, below): a chunk's copy in (h2d stream), kernels (stream) and copies out (d2h stream)
  // overlap its neighbours'.
  struct Work {
    dmi::DeviceBuffer scratch;     // [view][vertex] uchar4
    dmi::DeviceBuffer seeds;       // MedianSeed per vertex: what the projection pass hands the histogram-median pass
    dmi::DeviceBuffer margins[2];  // ViewMargin per view, for the chunk being processed
    dmi::DeviceBuffer pmax[2];     // launch_chunk_margins' four words
    hipEvent_t k0[2] = {nullptr, nullptr}, kdone[2] = {nullptr, nullptr};  // before / after a chunk's kernels: the kernel time
    hipEvent_t span[2] = {nullptr, nullptr};  // around all kernels of an in-place call, or of a round of the rasteriser
    size_t scratch_budget = size_t(1) << 30;  // bytes of scratch per chunk (dmi_color_set_scratch_budget)
    double last_kernel_ms = 0.0;
    void release() {
      dmi::free_buffers({&scratch, &seeds, &margins[0], &margins[1], &pmax[0], &pmax[1]});
      dmi::destroy_events(k0), dmi::destroy_events(kdone), dmi::destroy_events(span);
    }
  } work;
  struct Staging {  // what only the staged form (dmi_color_process) uses
    dmi::DeviceBuffer points[2], mean[2], median[2], count[2];
    hipStream_t h2d = nullptr, d2h = nullptr;
    hipEvent_t up[2] = {nullptr, nullptr}, down[2] = {nullptr, nullptr};  // copy in done / copies out done
    void release() {  // (the streams: dmi_color_destroy)
      dmi::free_buffers({&points[0], &points[1], &mean[0], &mean[1], &median[0], &median[1], &count[0], &count[1]});
      dmi::destroy_events(up), dmi::destroy_events(down);
    }
  } staging;
  // processing order of a chunk: Z-order keys and vertex indices (in / out of the radix sort), its temporary storage, the
  // chunk's bounding box; the in-place form's sample of vertices
  struct Order {
    dmi::DeviceBuffer keys, keys_sorted, index, perm, sort_temp, box, sample;
    size_t sort_temp_bytes = 0;  // what rocPRIM asked for at the key buffers' capacity: the size every sort is called with
    bool reorder = false;        // take the vertices of a chunk along a Z-order curve (dmi_color_set_vertex_reorder)
    void release() { dmi::free_buffers({&keys, &keys_sorted, &index, &perm, &sort_temp, &box, &sample}); }
  } order;
  // the rasteriser (dmi_color_render_depths, mesh_depth_render.hip): the planes of the last rendering -- ONE allocation for all
  // views, which then owns every entry of h_depth_planes --, the cameras as it reads them, its queue of large pairs and the
  // counters of a call (one per view group, then the id check's flag)
  struct Render {
    dmi::DeviceBuffer planes, cameras, queue, counters;
    uint32_t queue_capacity = 1u << 20;  // entries a call starts with (dmi_color_set_render_queue_capacity)
    std::vector<hipEvent_t> events;      // two around the fill, three per view group (before, between, after)
    double last_ms = 0.0;
    double last_pass_ms[3] = {0.0, 0.0, 0.0};  // the fill, the small passes, the large passes (dmi_color_get_render_pass_ms)
    uint64_t last_queued = 0;                  // (triangle, view) pairs the large passes took
    void release() {
      dmi::free_buffers({&planes, &cameras, &queue, &counters});
      for (hipEvent_t ev : events) (void)hipEventDestroy(ev);
      events.clear();
    }
  } render;
  struct Stage {  // the one staging buffer of the view uploads and the depth download
    dmi::DeviceBuffer buffer;
    void release() { dmi::free_buffers({&buffer}); }
  } stage;
};
