// Part of libcoreg_hip.so's ONE translation unit (coreg_hip.hip includes the parts in order; round 6 split by concern,
// no behaviour change): the per-launch fix arguments and the handle (coreg_handle): every field the ABI functions share,
// every buffer, event and stream an owning member (host_owned.hpp) -- there is no list of what to free.
#pragma once
namespace {

// where the pixels of an upload live
enum SrcKind {
    SRC_HOST = 0,    // pageable host memory: staged through the handle's pinned buffers
    SRC_PINNED = 1,  // page-locked host memory every device can DMA from (coreg_multi's shared staging): one async copy
    SRC_DEVICE = 2,  // memory of the handle's GPU: read where it is
    SRC_TILED = 3,   // a coreg_fits_tiled in host memory (the image to align): compressed bytes up, decoded on the GPU
};

// what the pixels of an upload are: native float32 / float64, or a FITS data unit's big-endian elements
struct PixFmt {
    int bitpix = 0;  // 0: native pixels (`f32` says which); else the FITS BITPIX of raw big-endian pixels
    bool f32 = false;
    double bscale = 1.0, bzero = 0.0;
    bool raw() const { return bitpix != 0; }
    bool scaled() const { return bscale != 1.0 || bzero != 0.0; }  // (as utils/fits_io.py decides it)
    size_t elem() const { return raw() ? (size_t)(bitpix < 0 ? -bitpix : bitpix) / 8 : (f32 ? 4 : 8); }
    bool swap_only() const { return bitpix == -32 && !scaled(); }  // decoded in place: float32 pixels
    static PixFmt native(bool is_f32) {
        PixFmt f;
        f.f32 = is_f32;
        return f;
    }
};

constexpr int kMaxDevices = 64;
std::mutex g_attr_mutex;

struct EventPair {
    Event a, b;
    bool b_is_next_sweep = false;  // precompute intervals end at the opening event of sweep launch `next_sweep_index`
    size_t next_sweep_index = 0;
};

}  // namespace

// The noise-decided samples of ONE launch as kernel arguments: run once about the global pivots into the
// launch's extra slab and -- when lag-points of the launch are re-evaluated -- a second time about the flagged slots'
// own pivots (launch_sweep, coreg_finalize_sums).  The device lists the arguments point to live until the next sweep.
// (a launch's single-sample lists kept past the next launch of the same sweep: grid-shared plate-carree sweeps)
struct KeptTapLists {
    DevBuf all;  // the five lists of TapFixArgs, one after another (keep_tap_lists)
};
// single samples near an integer coordinate: the device lists k_tap_fix reads (prepare_tap_fix fills them into the
// BorderFix of a launch, build_fix_launch adds the fields every fix kernel shares)
struct TapFix {
    TapFixArgs args = {};
    int segs = 0;         // lag-points listed = workgroups of k_tap_fix; 0: no single-sample pass
    int mode = 0;         // sweep mode the coordinates were scanned under (k_tap_fix<TS, mode>)
    long long count = 0;  // entries of the lists
};
struct FixLaunch {
    std::vector<BorderFixArgs> border;
    std::vector<ParityFixArgs> parity;
    TapFix tap;
    std::shared_ptr<KeptTapLists> kept;
    bool small_f32 = true;
    bool empty() const { return border.empty() && parity.empty() && tap.segs == 0; }
};

struct ContextState;  // frames and work space of the iterative-context sweep (host_context.hpp)
struct PixelsState;   // images and work space of the integer pixel-lag sweep (host_pixels.hpp)

// Ownership: every buffer, event and stream below frees itself when the handle is deleted; coreg_destroy is the one route
// there and keeps three invariants.  (1) Every stream is idle before anything is freed: it stops the upload thread and
// synchronizes `stream` and `up_stream` (`aux_stream` is synchronized by its one user before that returns).  (2) The
// handle's device is current while it is destroyed.  (3) A borrowed stream (coreg_set_stream) is never destroyed.
// With (1) no member needs another to outlive it, so the members stand in the order that reads best and ~coreg_handle
// has an empty body.
struct coreg_handle {
    int device = 0;
    Stream stream;  // the library's own, or the caller's (coreg_set_stream: borrowed)
    std::string err;

    std::unique_ptr<ContextState> ctx;  // created by coreg_set_context_frames
    std::unique_ptr<PixelsState> pix;   // created by the first coreg_pixels_* call that needs it (pixels_state)
    ~coreg_handle();                    // (defined where both are complete: coreg_hip.hip)

    // small image
    DevBuf small;
    int sW = 0, sH = 0;
    bool small_f32 = false;
    // reference on grid
    DevBuf ref;
    int gW = 0, gH = 0;
    int ref_dtype = -1;
    // pivots[0] = mean(reference), pivots[1] = mean(small)
    DevBuf pivots, red_sum, red_cnt;
    // geometry tables (+ the host copy they were built from: re-uploaded only when the grid changes)
    DevBuf t_sin_lon, t_cos_lon, t_cos_lat, t_sin_lat, t_lon_deg, t_dx;
    // differential rotation per role (coreg_set_reference_rotation / coreg_set_small_rotation); has_* false: off
    coreg_diffrot rot_ref = {}, rot_small = {};
    bool has_rot_ref = false, has_rot_small = false;
    // NaN-aware smoothing (host_smooth.hpp): the planes num and den of a call, the smoothed copy of an image (exchanged
    // with `small` by coreg_smooth_small; what the resample reads while the reference smoothing is set), and the tables of
    // coreg_set_reference_smoothing, which stay until set again or cleared
    DevBuf sm_num, sm_den, sm_out;
    std::vector<double> ref_smooth_y, ref_smooth_x;  // both empty: off
    // median/MAD despiking (host_despike.hpp): the two buffers its passes write in turn (the last one is exchanged with
    // `small` by coreg_despike_small; what the smoothing or the resample reads while the reference despiking is set), the
    // flagged counts uint64 [2][8] on the device (image / last reference preparation), the parameters of
    // coreg_set_reference_despike, which stay until set again or cleared, and the passes of the last preparation
    DevBuf ds_a, ds_b, ds_counts;
    coreg_despike_params ref_despike = {};
    bool has_ref_despike = false;
    int ref_despike_passes = 0;
    // despiking and summing a stack of planes (host_despike_planes.hpp): buffers of its own, so that a call leaves the
    // resident images and the reference despiking as they were -- the page-locked staging of the selected planes, the
    // stack as the file stores it, the two stacks its passes before the last write in turn, the sum, the event map and
    // the flag events per pass uint64 [8], the time of the last call's kernels; "despike_planes_overlap" 0: the last pass
    // stages every plane before it decides it (what the overlap is timed against)
    PinBuf dp_pin;
    DevBuf dp_raw, dp_a, dp_b, dp_sum, dp_events, dp_counts;
    Event dp_ev[2];          // around the passes of a call (created by the first one)
    double dp_last_ms = -1;  // the passes of the last call by those events, upload and read-back left out; < 0: no call yet
    int64_t opt_despike_planes_overlap = 1;
    CarrTables tabs;
    std::vector<double> tabs_key;
    bool tabs_uploaded = false;  // the device tables are those of `tabs`
    PinBuf pin_img[2];
    Event ev_img[2];
    int pin_img_next = 0;
    // precompute outputs
    DevBuf pts, tile_count, tile_list, tile_cum, group_first, tile_info, tile_bbox;
    DevBuf visit_rec;  // [non-empty tiles + 1] VisitRec: what k_sweep reads per tile visit (k_tile_list)
    DevBuf rf_fix_slab;  // [kNumSums][n_slots]: a launch's noise-decided samples about the flagged slots' own pivots
    DevBuf counters;  // [0]: lag-points re-evaluated by k_finalize during the sweep in flight (reset by its prologue)
    // sweep
    DevBuf lane_params, out_index, partials, out_dev, tmp_img;
    // k_sweep's persistent workgroups (launch_sweep): the eight ticket counters of a launch, zeroed on the handle's stream
    // before every launch; the compute units of the device; and how many workgroups of an instantiation one of them
    // holds at a given dynamic-LDS size, asked of the runtime once per (kernel, bytes)
    DevBuf sweep_queue;
    int n_cus = 0;
    struct SweepResidency {
        const void* fn;
        size_t lds_bytes;
        int per_cu;
    };
    std::vector<SweepResidency> sweep_residency;
    int64_t opt_sweep_wgs = 0;  // "sweep_wgs": workgroups a k_sweep launch may have resident; 0: CUs x workgroups per CU
    // per-lag sample counts of the last sweep / coreg_finalize_sums / coreg_sweep_context call, laid out like its output
    // (coreg_last_counts); counts_n < 0: no such call yet
    DevBuf counts;
    long long counts_n = -1;
    DevBuf up_f64, up_flag;  // upload staging on the device (float64 copy, exactness flag)
    DevBuf up_raw;           // raw FITS elements awaiting their decode (BITPIX other than an unscaled -32)
    DevBuf rice_blob, rice_rand, dec_img;  // tile-compressed images: heap + tile tables, cfitsio's random sequence, a
                                           // decoded reference image (the image to align is decoded in place)
    PrologueArgs pending_prologue = {};  // set by upload_plan, consumed by the sweep's first k_precompute launch
    DevBuf bbox_buf;         // reference_crop: partial bounding boxes
    Stream aux_stream;  // side stream of reference_crop (created on first use)
    // The image to align goes up on a stream of its own (round 5): the preparation of the reference image -- bounding
    // box, crop upload, resample -- depends on headers and the reference image only and no longer queues behind the
    // 16 MiB of the image to align; the first call that reads the image (or its pivot) joins the two streams with an event
    // (bind_device).  float32 / byte-swap-only uploads from host memory; everything else stays on `stream`.
    Stream up_stream;
    Event ev_small, ev_main;
    bool small_pending = false;
    DevBuf red_sum_up, red_cnt_up;  // device_mean's scratch on up_stream
    int64_t opt_overlap_upload = 1;
    int64_t opt_tap_nan_filter = 2;  // odd orders: list only the near-integer samples that can change the result (k_tap_scan);
                                     // 1: a non-finite pixel anywhere in the union of the footprints, 2: + the sharper
                                     // end-line test where one axis only is near an integer, 0: list them all
    // "async_upload" (opt-in: the caller's image buffer must stay valid and unchanged until the next call that reads the
    // image returns): the staging copies + DMA of coreg_set_small_f32 / _fits run on a worker thread of the handle, so that
    // the calling thread goes on to prepare the reference and plan the sweep meanwhile; joined before the first kernel
    // that reads the image (join_small).  Staging and events of its own: nothing is shared with the calling thread.
    int64_t opt_async_upload = 0;
    std::thread up_thread;
    std::mutex up_m;
    std::condition_variable up_cv;
    std::function<hipError_t()> up_job;
    bool up_has = false, up_stop = false, up_busy = false;
    hipError_t up_rc = hipSuccess;
    PinBuf pin_small[2];
    Event ev_pin_small[2];
    int pin_small_next = 0;
    // zero-lag border decisions of the sub-map paths, cached per header pair (sweep_plan.hpp: the planners are handed it)
    WcslibCaches wcslib;
    DevBuf border_flags, fix_partial;
    DevBuf border_dev;
    PinBuf pin_border;
    int64_t opt_border_fix = 1;
    // odd spline orders, general case: samples whose coordinate comes back within opt_tap_tol of an integer are
    // re-evaluated with wcslib's own arithmetic (k_tap_scan / k_tap_fix)
    int64_t opt_tap_fix = 1, opt_tap_cap = 1 << 24;
    DevBuf tap_count, tap_segq, tap_list, tap_skip, tap_seg_slot, tap_seg_begin, tap_pixel, tap_xw, tap_yw;
    long long tap_last[3] = {0, 0, 0};  // last sweep: samples listed, lag-points concerned, 1 = list overflowed (no fix)
    // the k_sweep instantiation of the last launch of the last sweep (coreg_last_sweep_variant): index in
    // sweep_variant::kSweepVariants, mode, order, f32, round, resid, pitch; index -1: that sweep launched none
    int last_variant[7] = {-1, 0, 0, 0, 0, 0, 0};
    // multi-GPU point sharding (coreg_set_option "shard_world" / "shard_rank"): a sweep covers this rank's share of the
    // tile groups and leaves the six sums per lag slot in `sums`; coreg_finalize_sums turns the all-reduced sums into
    // coefficients
    int64_t opt_shard_world = 1, opt_shard_rank = 0;
    // multi-GPU combination sharding ("combo_begin" / "combo_end"): the NEXT sweep covers only the (cdelt1, cdelt2, crota)
    // combinations [begin, end) of the lag set's inner C-order index; consumed (reset to "all") by that sweep
    int64_t opt_combo_begin = 0, opt_combo_end = 0;
    DevBuf sums;
    long long sums_slots = 0;  // slots of the pending sharded sweep (all its launches)
    struct PendingFinalize {
        long long slot_off, n_slots, lag_begin;
        int residus;
        // what coreg_finalize_sums needs to re-evaluate the ill-conditioned lag-points of this launch once the ranks' sums
        // are added (the flags come from the REDUCED sums): the launch's refine arguments and, when later launches of the
        // same sweep have overwritten the compacted points, how to compute them again
        RefineArgs refine;
        std::function<int(coreg_handle*)> replay_precompute;
        FixLaunch fixes;  // the launch's noise-decided samples, for the second run about the flagged slots' pivots
    };
    std::function<int(coreg_handle*)> last_precompute;  // the precompute launch the next launch_sweep follows
    PlanMemo plan_memo;  // the last lag plan and what it was made from (sweep_plan.hpp choose_plan)
    DevBuf rf_flags, rf_pivots, rf_list, rf_head, rf_partial;  // work space of the re-evaluation (kernels.hpp: RefineArgs)
    std::vector<PendingFinalize> pending_fin;
    DevBuf fin_outidx;        // copy of the output indices of the pending sharded sweep
    long long pending_n_out = 0;
    // COREG_METHOD_MUTUAL_INFORMATION of coreg_sweep_carrington (host_sweep_mi.hpp): the edge lists of
    // coreg_sweep_set_bins, kept until set again (a state of their own: coreg_pixels_set_bins has the pixel-lag sweep's);
    // the global histograms uint32 [slot][cell] of a launch, zeroed per launch and sized by the largest one; the dynamic
    // LDS each k_sweep_mi instantiation has been allowed on this handle's device so far
    std::vector<double> mi_edges_small, mi_edges_large;
    DevBuf mi_hist;
    size_t mi_lds[6] = {0, 0, 0, 0, 0, 0};
    int64_t opt_mi_chunks = 0;  // chunks of the tile list per group of 16 lag slots; 0: the planner's choice

    // options
    int64_t opt_crop_reference = 1;
    int64_t opt_taper_min = 128, opt_taper_frac = -1, opt_taper_rounds = 6;  // tapered group shares (pick_taper)
    int64_t opt_use_lds = 1, opt_clean_path = 1, opt_refine = 1, opt_refine_cond_log10 = 5, opt_tile_w = 0, opt_n_groups = 0, opt_lds_bytes = (159 * 1024 * kPointGroups) / 4, opt_patch_w = 0, opt_h_series = 1, opt_h_incr = 1, opt_tile_skip = 1, opt_pitch = -1;

    coreg_stats stats;
    bool stats_pending = false;   // a device-output sweep is in flight: timings are collected on demand
    PinBuf pin_info;              // tile_info read-back of the in-flight sweep
    std::vector<EventPair> ev_sweep, ev_pre;
    size_t ev_sweep_used = 0, ev_pre_used = 0;
    hipEvent_t ev_t1 = nullptr;  // (not owned)
    // The plan staging (lag parameters in pinned memory) is double-buffered: slot k is rewritten only when the sweep
    // that last used it has ended (its end event), so the host can plan sweep n + 1 while the GPU runs sweep n, with no
    // extra event between the kernels.  ev_t1 is an alias of the current slot's end event.
    Event ev_end[2];
    PinBuf pin_plan[2];
    int plan_slot = 0;
    bool plan_open = false;  // upload_plan has staged a plan that no end_sweep has closed yet (a sweep that failed midway)
};

