// c3_hostring.h -- the host <-> device side of the model call: c3_predict (the reference's blocking _torch_predict,
// clair3/CallVariantsFromCffi.py:48-52), its asynchronous pair c3_predict_submit / c3_predict_wait (a ring of C3_HOST_SLOTS
// batches in flight: staging copy, H2D, kernels, D2H, range guard), the region form of the pileup call, and the decoder entry
// points that take host rows.  The library never page-locks CALLER memory (see stage_h2d).
#pragma once
#include "c3_forward.h"

// ------------------------------------------------------------------------------------------ host staging
// The caller's windows are pageable numpy memory (clair3/CallVariantsFromCffi.py:112-133: np.load slices); they go
// through a pinned buffer, cut into pieces: the H2D transfer of a piece is queued as soon as it is staged, so the DMA of
// piece i runs under the memcpy of piece i + 1, and every piece's memcpy is split over the staging pool (c3_host.h).
// There is NO zero-copy source path: until round 5 the ABI could page-lock caller memory (hipHostRegister: c3_host_register,
// c3_model_set_lock_sources).  On ROCm 7.2 a process that registers / unregisters host ranges and also lets another HIP user (PyTorch)
// copy from pageable memory takes "Memory access fault by GPU" sooner or later (tests/diag/register_vs_torch_probe.py reproduces it
// with hipHostRegister and torch alone), and a C ABI cannot know who else lives in its process: the entry points are gone, every
// caller buffer -- numpy, a memory-mapped tensor file, libclair3's fa_data.matrix -- is staged through the library's own pinned,
// MADV_DONTFORK memory.  Price: 0.86 instead of 0.88 of the device-resident rate on a blocking call of 1000 full-alignment windows.

// Rows always leave through a copy kernel on the COMPUTE stream (host_copy_kernel writes the pinned, device-mapped result
// buffer): handing them to a transfer stream -- event, cross-queue wait, DMA copies, event -- cost the compute queue ~75 us per
// batch (profiles/r03_e_d2h_by_kernel.txt).  Windows come in on the transfer stream (DMA engine; the compute stream's wait for
// that event is free, the transfer finished batches ago) -- except a batch in a lane, which stages them on its lane's own stream,
// and a small batch with nothing else in flight (the blocking call of one chunk): there a copy kernel on the compute stream
// reading the pinned staging buffer is the shorter way, up to kKernelCopyMax bytes (4000 pileup windows = 2.4 MB, ~50 us at
// PCIe Gen5 rates).
constexpr size_t kKernelCopyMax = (size_t)4 << 20;
__global__ __launch_bounds__(256) void host_copy_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst, size_t n16,
                                                       const uint32_t *flag_src, uint32_t *flag_dst) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) dst[i] = src[i];
    if (flag_dst && blockIdx.x == 0 && threadIdx.x == 0) *flag_dst = *flag_src;
}

// one thread per output float: raises the handle's range flag when a probability is not finite
__global__ void rows_finite_kernel(const float *y, int64_t n, uint32_t *flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && (__float_as_uint(y[i]) & 0x7f800000u) == 0x7f800000u) atomicOr(flag, 2u);
}

// workgroups of the copy kernel that writes the rows into the pinned result buffer: 32 for a batch (96 KB), up to 256 for a group
// of 2000 full-alignment rows with decoder columns (968 KB): more stores in flight across PCIe
static unsigned rows_out_grid(size_t bytes) { return (unsigned)std::min<size_t>(256, std::max<size_t>(32, bytes / 4096)); }

// stage [src, src + bytes) through `pin` into `dev` on stream s, piecewise
static int stage_h2d(void *dev, void *pin, const void *src, size_t bytes, hipStream_t s) {
    // >= 4 MiB and at most four pieces: every queued transfer costs ~15 us of host time (2 MiB x 8 was slower again)
    const size_t piece = std::max<size_t>((size_t)4 << 20, ((bytes / 4) + 4095) & ~(size_t)4095);
    for (size_t off = 0; off < bytes; off += piece) {
        const size_t n = std::min(piece, bytes - off);
        StagePool::get().copy((char *)pin + off, (const char *)src + off, n);
        HIP_TRY(hipMemcpyAsync((char *)dev + off, (char *)pin + off, n, hipMemcpyHostToDevice, s));
    }
    return 0;
}

// ------------------------------------------------------------------------------------------ occupied rows of full-alignment windows (c3_expand.h)
// entry i of a caller's int32 table that may sit at any byte address
static inline int32_t table_i32(const int32_t *p, int64_t i) {
    int32_t v;
    memcpy(&v, (const char *)p + 4 * i, 4);
    return v;
}
// wide ORs over a row; stops at the first 32 bytes that hold a set bit (p may sit at any byte address)
static inline bool row_is_zero(const uint8_t *p, size_t n) {
    size_t i = 0;
    for (; i + 32 <= n; i += 32) {
        uint64_t a, b, c, d;
        memcpy(&a, p + i, 8), memcpy(&b, p + i + 8, 8), memcpy(&c, p + i + 16, 8), memcpy(&d, p + i + 24, 8);
        if ((a | b) | (c | d)) return false;
    }
    uint64_t acc = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t a;
        memcpy(&a, p + i, 8);
        acc |= a;
    }
    for (; i < n; ++i) acc |= p[i];
    return acc == 0;
}
// the run from the first to the last non-zero row of a dense window (interior zero rows stay inside it; an all-zero window: count 0, first
// 0): scanned from the top and from the bottom, so only zero rows and the two boundary rows are read
static inline void occupied_run(const uint8_t *w, int depth, size_t row_bytes, int32_t *first, int32_t *count) {
    int top = 0;
    while (top < depth && row_is_zero(w + (size_t)top * row_bytes, row_bytes)) ++top;
    if (top == depth) {
        *first = 0, *count = 0;
        return;
    }
    int bot = depth - 1;
    while (row_is_zero(w + (size_t)bot * row_bytes, row_bytes)) --bot;
    *first = top, *count = bot - top + 1;
}

// ------------------------------------------------------------------------------------------ candidate selection (c3_select.h)
static int run_select(c3_model *m, hipStream_t s, const SelectParams &sp) {
    ProfScope ps(m, s, "p.select", 0.0, 4.0 * sp.n_cand * (double)(sp.T * sp.C));
    const dim3 grid((unsigned)((sp.n_cand + kSelectThreads / 64 - 1) / (kSelectThreads / 64)));
    if (sp.C % 2 == 0) hipLaunchKernelGGL(candidate_status_kernel<2>, grid, dim3(kSelectThreads), 0, s, sp);
    else hipLaunchKernelGGL(candidate_status_kernel<1>, grid, dim3(kSelectThreads), 0, s, sp);
    HIP_TRY(hipGetLastError());
    const dim3 tiles((unsigned)((sp.n_cand + kCompactTile - 1) / kCompactTile));
    hipLaunchKernelGGL(kept_count_kernel, tiles, dim3(kCompactTile), 0, s, sp);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(compact_kept_kernel, tiles, dim3(kCompactTile), 0, s, sp);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" {

// Pinned staging memory stays out of forked children (keep_out_of_children, c3_model.h: the staging copies of the 40 groups after
// eight forks 155 -> 97 ms, profiles/r05_k_host_loop_feeder_not_kept.txt).
static int ensure_slot(HostSlot &sl, size_t xb, size_t yb) {
    // host_copy_kernel moves whole 16-byte pieces ((bytes + 15) / 16 of them): every buffer it touches is sized to a multiple of
    // 256 bytes here, for every path (90-column rows of an odd batch, 121-float decoder rows: yb % 16 != 0) -- and to whole pages, so that
    // the pinned halves can be kept out of forked children page by page (keep_out_of_children)
    xb = (xb + 4095) & ~(size_t)4095, yb = (yb + 4095) & ~(size_t)4095;
    if (!sl.ev_h2d) {
        HIP_TRY(hipEventCreateWithFlags(&sl.ev_h2d, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&sl.ev_out, hipEventDisableTiming));
    }
    if (!sl.pin_flag) {
        HIP_TRY(hipHostMalloc((void **)&sl.pin_flag, 4096, hipHostMallocDefault));  // (a whole page: MADV_DONTFORK works on pages)
        keep_out_of_children(sl.pin_flag, 4096);
    }
    if (xb > sl.cap_x) {
        if (sl.pin_x) (void)hipHostFree(sl.pin_x);
        if (sl.dev_x) (void)hipFree(sl.dev_x);
        sl.pin_x = sl.dev_x = nullptr, sl.cap_x = 0;
        HIP_TRY(hipHostMalloc(&sl.pin_x, xb, hipHostMallocDefault));
        keep_out_of_children(sl.pin_x, xb);
        HIP_TRY(hipMalloc(&sl.dev_x, xb));
        sl.cap_x = xb;
    }
    if (yb > sl.cap_y) {
        if (sl.pin_y) (void)hipHostFree(sl.pin_y);
        if (sl.dev_y) (void)hipFree(sl.dev_y);
        sl.pin_y = nullptr, sl.dev_y = nullptr, sl.cap_y = 0;
        HIP_TRY(hipHostMalloc((void **)&sl.pin_y, yb, hipHostMallocDefault));
        keep_out_of_children(sl.pin_y, yb);
        HIP_TRY(hipMalloc((void **)&sl.dev_y, yb));
        sl.cap_y = yb;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------ what a batch of the ring reads
enum class InKind {
    Sliced,      // x: the windows themselves
    Region,      // x: ONE region matrix of n_cols columns, window b starts at column starts[b] (checked against n_cols by the caller)
    Candidates,  // x: the region matrix, the starts are worked out on the device (c3_select.h); n_cols = columns of the device image
    Rows,        // full alignment: x holds the occupied rows of the windows back to back, row_count[b] of them for window b from dense row
                 // row_first[b] on (nullptr: centred, (depth - row_count[b]) / 2); checked by the caller, which also adds the counts up
    PackedHere,  // C3HIP_PACK_ROWS=1: sliced int8 full-alignment windows, packed into their occupied rows while they are staged (c3_expand.h)
    Parts,       // the windows themselves, in n_parts host buffers of counts[i] windows each: laid behind each other in the image section, so
                 // the batch the device sees is the plain batch of their concatenation; rows leave to y_parts[i] (c3_predict_submit_parts)
};
// candidate positions instead of window starts (c3_predict_submit_candidates): what the host knows of the region before it is staged
struct CandInput {
    const int64_t *pos = nullptr;     // [batch]
    bool head_tail = false;           // the device image carries positions - 1 zero columns in front of and behind every chunk
    std::vector<SelectChunk> chunks;  // col: the chunk's first column in the device image
    std::vector<int64_t> src_col;     // ... and in the caller's matrix
    uint8_t *status_host = nullptr;
    int64_t *n_rows_host = nullptr;
    // the region matrix already lies on this device (c3_predict_submit_pileup, c3_pileup.h): int32 columns in the order of the chunks.  Nothing
    // of it is staged: it reaches the slot by device-to-device copies on the lane's stream, behind the event of the stream that wrote it
    const void *dev_image = nullptr;
    hipEvent_t dev_ready = nullptr;
    hipEvent_t dev_taken = nullptr;  // recorded on the lane's stream behind those copies: the image's owner may overwrite it from there on
};
struct RingInput {
    InKind kind = InKind::Sliced;
    const void *x = nullptr;
    int x_dtype = C3_DTYPE_I8;  // of the STAGED counts
    int64_t batch = 0;
    float *y_host = nullptr, *y_dev = nullptr;  // where the rows go: this host, or (c3_predict_submit_dev) the caller's device buffer
    const int32_t *depth = nullptr;  // per-window depths: windows deeper than 1.5 x max_depth are rescaled on the device (c3_rescale.h)
    bool piece = false;              // a piece of a blocking call: its rescaled windows add to the call's count
    int64_t n_cols = 0;                                         // Region / Candidates
    const int32_t *starts = nullptr;                            // Region
    bool narrow = false;  // Region / Candidates: x holds int64 / size_t counts, narrowed to int32 on their way into the staging buffer
    const CandInput *cand = nullptr;                            // Candidates
    const int32_t *row_first = nullptr, *row_count = nullptr;  // Rows
    int64_t rows_total = 0;
    // Rows whose bytes already lie on this device (c3_predict_submit_fa_reads, c3_fa_reads.h): nothing of them is staged, they reach the slot
    // by one device-to-device copy on the lane's stream behind dev_ready; dev_taken is recorded behind that copy (their owner may overwrite)
    const void *dev_rows = nullptr;
    hipEvent_t dev_ready = nullptr, dev_taken = nullptr;
    const void *const *parts = nullptr;  // Parts
    const int64_t *counts = nullptr;
    float *const *y_parts = nullptr;
    int n_parts = 0;
    bool score = false;  // a scored batch (c3_score_submit; Sliced only): labels (batch, nout) of label_dtype; y_host may be nullptr (the rows stay
    const void *labels = nullptr;  // on the device), loss_host too (nobody asked for the windows' values)
    int label_dtype = C3_DTYPE_I8;
    float *loss_host = nullptr;
};
static RingInput ring_input(InKind kind, const void *x, int x_dtype, int64_t batch, float *y_host, const int32_t *depth = nullptr, float *y_dev = nullptr) {
    RingInput in;
    in.kind = kind, in.x = x, in.x_dtype = x_dtype, in.batch = batch, in.y_host = y_host, in.depth = depth, in.y_dev = y_dev;
    return in;
}
static bool is_rows(InKind k) { return k == InKind::Rows || k == InKind::PackedHere; }

// what every entry of the ring refuses first: a handle or slot that cannot take a batch (c3_predict_wait: that cannot hold one)
static int ring_ready(const c3_model *m, int slot, bool to_submit = true) {
    if (!m) return fail("null model");
    if (slot < 0 || slot >= kHostSlots) return fail("slot must be in [0, %d)", kHostSlots);
    if (!to_submit) return 0;
    if (m->slot[slot].busy) return fail("slot %d still in flight: call c3_predict_wait first", slot);
    if (!m->loaded) return fail("model has no weights: call c3_model_load first");
    return 0;
}

// ------------------------------------------------------------------------------------------ submit, step by step
// Beside batches in the other lanes: the kernel forms for a shared chip (c3_model.h lane_sharing; rows bit-identical either way) -- when this
// batch and the largest ones in flight in the other lanes would, on half tiles (two workgroups per 8 windows), ask for more workgroups than
// the chip has CUs (ring of 1024-window batches: yes; the blocking call's 250 + 750 pieces: no, 252 half-tile workgroups fit side by side).
// In force from here until submit returns, on any path.
struct LaneSharing {
    c3_model *m;
    LaneSharing(c3_model *m_, int64_t batch, bool beside) : m(m_) {
        int64_t other[kHostSlots], beside_windows = 0;
        int no = 0;
        for (int k = 0; beside && k < kHostSlots; ++k)
            if (m->slot[k].busy && m->slot[k].batch <= m->lane_max_batch) other[no++] = m->slot[k].batch;
        std::sort(other, other + no, std::greater<int64_t>());
        for (int k = 0; k < no && k < m->ring_lanes - 1; ++k) beside_windows += other[k];
        m->lane_sharing = (beside_windows > 0 && 2 * ((batch + beside_windows + 7) / 8) > m->wg_slots / 2) ? m->ring_lanes : 1;
        m->lane_beside = beside_windows > 0;
    }
    ~LaneSharing() { m->lane_sharing = 1, m->lane_beside = false; }
};

// the depths the batch stages; counts the windows the rule rescales (depth > 0 and depth > 1.5 x max_depth) for c3_model_describe.  A batch
// without a deep window runs exactly what it runs without depths: no pre-pass, no copy
static const int32_t *deep_depths(c3_model *m, const RingInput &in) {
    int64_t n_deep = 0;
    for (int64_t i = 0; in.depth && i < in.batch; ++i) n_deep += in.depth[i] > 0 && (double)in.depth[i] > 1.5 * (double)m->max_depth;
    m->rescaled = (in.piece ? m->rescaled : 0) + n_deep;
    return n_deep > 0 ? in.depth : nullptr;
}

// THE layout of a staged batch (c3_model.h StagedBatch), for every kind: nothing else computes an offset.  The kernels' alignment
// assumptions hang on it: sections from multiples of 256 bytes, the 8-byte pieces of expand_rows_kernel, the 16-byte pieces of host_copy_kernel
static StagedBatch plan_batch(const c3_model *m, const RingInput &in, bool with_depth, bool verify = false, bool layers = false, bool refine = false) {
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const bool cand = in.kind == InKind::Candidates, region = cand || in.kind == InKind::Region, rows = is_rows(in.kind);
    const size_t n = (size_t)in.batch, db = with_depth ? n * sizeof(int32_t) : 0;
    StagedBatch p;
    p.image.bytes = region ? (size_t)in.n_cols * m->C * (in.x_dtype == C3_DTYPE_I32 ? 4 : 1)
                    : in.kind == InKind::Rows ? (size_t)in.rows_total * m->positions * m->C : (size_t)(in.batch * c3_model_window_bytes(m, in.x_dtype));
    if (cand) p.cand_pos.bytes = n * sizeof(int64_t), p.depth_in.bytes = db, p.chunks.bytes = in.cand->chunks.size() * sizeof(SelectChunk);
    if (cand) p.start_all.bytes = n * sizeof(int32_t), p.tiles.bytes = (size_t)((in.batch + kCompactTile - 1) / kCompactTile) * sizeof(uint32_t);
    p.starts.bytes = region ? n * sizeof(int32_t) : 0, p.depth.bytes = db;
    if (rows) p.rows_tab.bytes = n * sizeof(ExpandEntry);  // (a batch packed here may need less than this bound: fill_packed_rows)
    if (in.score) p.labels.bytes = n * m->nout * (in.label_dtype == C3_DTYPE_F32 ? sizeof(float) : 1);
    size_t end = 0;
    for (Section *s : {&p.image, &p.cand_pos, &p.depth_in, &p.chunks, &p.starts, &p.depth, &p.start_all, &p.tiles, &p.rows_tab, &p.labels})
        s->off = al(end), end = s->off + s->bytes;
    // a candidate batch stages up to its chunk table: the arrays behind it are written by the selection kernels
    p.tail = rows ? p.rows_tab.off : p.cand_pos.off;
    p.staged = cand ? p.chunks.off + p.chunks.bytes
               : rows || p.labels.bytes ? end : (p.starts.bytes + p.depth.bytes ? p.depth.off + p.depth.bytes : p.image.bytes);
    p.x_cap = cand ? end : p.staged;
    // ... and its statuses and the count of kept candidates leave behind the rows
    p.y.bytes = n * m->row * sizeof(float);
    p.status.off = al(p.y.bytes), p.status.bytes = cand ? n : 0;
    p.kept.off = p.status.off + ((n + 15) & ~(size_t)15), p.kept.bytes = cand ? 16 : 0;
    p.y_total = cand ? p.kept.off + p.kept.bytes : p.y.bytes;
    // ... and a verified batch's record (c3_verify.h) behind them; rows that stay on the device: the record is all the slot's output buffer holds
    if (verify) p.verify.off = in.y_dev ? 0 : al(p.y_total), p.verify.bytes = kVerifyRecordBytes, p.y_total = p.verify.off + p.verify.bytes;
    // ... and its layer records (c3_model_set_verify_layers) behind that
    if (verify && layers) p.layers.off = p.y_total, p.layers.bytes = kLayerRecordsBytes, p.y_total = p.layers.off + p.layers.bytes;
    // ... and a scored batch's record (c3_score.h) behind everything else, the windows' values behind the record when the caller wants them
    if (in.score) {
        p.score.off = al(p.y_total), p.score.bytes = kScoreRecordBytes, p.y_total = p.score.off + p.score.bytes;
        if (in.loss_host) p.losses.off = p.y_total, p.losses.bytes = n * (size_t)m->nb * sizeof(float), p.y_total = p.losses.off + p.losses.bytes;
        // ... and, only while the handle's census is on (c3_census.h), the batch's table behind those
        if (m->score_census_on) p.census.off = al(p.y_total), p.census.bytes = kScoreCensusBytes, p.y_total = p.census.off + p.census.bytes;
    }
    // ... and, only while refine mode is on and covers the batch (c3_refine.h; never together with a verify record), its record and the list of
    // selected windows behind everything else; rows that stay on the device: all the slot's output buffer holds
    if (refine)
        p.refine.off = in.y_dev ? 0 : al(p.y_total), p.refine.bytes = kRefineRecordBytes + ((n * sizeof(int32_t) + 15) & ~(size_t)15),
        p.y_total = p.refine.off + p.refine.bytes;
    return p;
}

// ---- fill the pinned buffer: one function per kind.  What is left for the transport: the image either still sits in the caller's memory
// (src: it passes through the pinned buffer piece by piece, every piece's transfer queued as soon as it is copied, stage_h2d) or is
// already in the pinned buffer as nrun runs
struct Filled {
    const void *src = nullptr;
    int nrun = 0;
    struct Run { size_t off, bytes; } run[8];
    int64_t rows_shipped = 0;
    bool no_image = false;  // the image section is filled on the device (queue_device_image): nothing of it crosses from the pinned buffer
    void prebuilt(size_t bytes) { nrun = 1, run[0] = Run{0, bytes}; }
};
// int64 = plp_data.matrix itself (size_t counts, src/clair3_pileup.h:113): narrowed to int32 on its way into the staging
// buffer, which is what the reference's PIPE mode feeds the model (CreateTensorPileupFromCffi.py:143-146 -> int32 windows)
static void narrow_counts(int32_t *dst, const int64_t *src, size_t n) {
    for (size_t i = 0; i < n; ++i) dst[i] = (int32_t)src[i];
}
// the region matrix as ONE image: narrowed here, or left to the transport
static void fill_region_image(const c3_model *m, const HostSlot &sl, const RingInput &in, const StagedBatch &p, Filled &f) {
    if (!in.narrow) f.src = in.x;
    else narrow_counts(static_cast<int32_t *>(sl.pin_x), static_cast<const int64_t *>(in.x), (size_t)in.n_cols * m->C), f.prebuilt(p.image.bytes);
}
static void fill_sliced(const HostSlot &sl, const RingInput &in, const StagedBatch &p, const int32_t *depth, Filled &f) {
    if (depth) memcpy(sl.pin<char>(p.depth), depth, p.depth.bytes);
    f.src = in.x;
}
// a scored batch: its labels behind whatever else it stages
static void fill_labels(const HostSlot &sl, const RingInput &in, const StagedBatch &p) {
    if (p.labels.bytes) memcpy(sl.pin<char>(p.labels), in.labels, p.labels.bytes);
}
// parts: each caller buffer gets the one copy every caller buffer gets, part i behind part i - 1 in the image section
static void fill_parts(const HostSlot &sl, const RingInput &in, const StagedBatch &p, size_t window_bytes, Filled &f) {
    size_t off = p.image.off;
    for (int i = 0; i < in.n_parts; ++i) {
        const size_t n = (size_t)in.counts[i] * window_bytes;
        if (n) StagePool::get().copy((char *)sl.pin_x + off, in.parts[i], n);
        off += n;
    }
    f.prebuilt(p.image.bytes);
}
// ... and c3_predict_wait's way back: the rows of part i, in batch order, to where its caller wants them
static void scatter_parts(const HostSlot &sl, size_t row_bytes) {
    const char *src = (const char *)sl.pin_y + sl.plan.y.off;
    for (int i = 0; i < sl.n_parts; ++i) {
        const size_t n = (size_t)sl.part_count[i] * row_bytes;
        if (n) memcpy(sl.part_y[i], src, n);
        src += n;
    }
}
static void fill_region(const c3_model *m, const HostSlot &sl, const RingInput &in, const StagedBatch &p, const int32_t *depth, Filled &f) {
    memcpy(sl.pin<char>(p.starts), in.starts, p.starts.bytes);
    if (depth) memcpy(sl.pin<char>(p.depth), depth, p.depth.bytes);
    fill_region_image(m, sl, in, p, f);
}
static void fill_candidates(const c3_model *m, const HostSlot &sl, const RingInput &in, const StagedBatch &p, const int32_t *depth, Filled &f) {
    const CandInput &ci = *in.cand;
    memcpy(sl.pin<char>(p.cand_pos), ci.pos, p.cand_pos.bytes);
    if (depth) memcpy(sl.pin<char>(p.depth_in), depth, p.depth_in.bytes);
    memcpy(sl.pin<char>(p.chunks), ci.chunks.data(), p.chunks.bytes);
    if (ci.dev_image) {  // (queue_device_image brings the image in)
        f.no_image = true;
        return;
    }
    if (!ci.head_tail) return fill_region_image(m, sl, in, p, f);
    // head / tail windows: the image is laid out in the staging buffer chunk by chunk, positions - 1 zero columns in front of and behind
    // each (c3_select.h)
    const size_t colb = (size_t)m->C * sizeof(int32_t), pad = (size_t)(m->positions - 1);
    for (size_t k = 0; k < ci.chunks.size(); ++k) {
        const SelectChunk &ch = ci.chunks[k];
        const size_t n = (size_t)(ch.last - ch.first + 1), c0 = (size_t)ch.col, s0 = (size_t)ci.src_col[k];
        int32_t *dst = (int32_t *)((char *)sl.pin_x + c0 * colb);
        memset((char *)sl.pin_x + (c0 - pad) * colb, 0, pad * colb);
        if (in.narrow) narrow_counts(dst, static_cast<const int64_t *>(in.x) + s0 * m->C, n * m->C);
        else StagePool::get().copy(dst, (const char *)in.x + s0 * colb, n * colb);
        memset((char *)sl.pin_x + (c0 + n) * colb, 0, pad * colb);
    }
    f.prebuilt(p.image.bytes);
}
// rows handed over: the table of {source byte offset, first dense row, rows} per window, filled in one pass over the counts
static void fill_rows(const c3_model *m, const HostSlot &sl, const RingInput &in, const StagedBatch &p, Filled &f) {
    ExpandEntry *tab = sl.pin<ExpandEntry>(p.rows_tab);
    int64_t o = 0, row_bytes = (int64_t)m->positions * m->C;
    for (int64_t b = 0; b < in.batch; ++b) {
        const int32_t c = table_i32(in.row_count, b);
        tab[b] = ExpandEntry{o, in.row_first ? table_i32(in.row_first, b) : (m->depth - c) / 2, c};
        o += (int64_t)c * row_bytes;
    }
    f.rows_shipped = in.rows_total;
    if (in.dev_rows) f.no_image = true;  // (queue_device_rows brings the rows in)
    else f.src = in.x;
}
// rows packed here: the scan of c3_pack_rows writes every window's run straight into the pinned buffer, split over the staging pool by window
// ranges: range k packs back to back from where its first window would start in the dense layout (an 8-byte boundary for an even C), so no
// range waits for the count of the one before it and the runs cross PCIe as one transfer per range.  ONE range: the table moves up behind
// its rows (the plan is settled here)
static void fill_packed_rows(const c3_model *m, const HostSlot &sl, const RingInput &in, StagedBatch &p, Filled &f) {
    const size_t row_bytes = (size_t)m->positions * m->C, wbytes = (size_t)m->depth * row_bytes;
    std::vector<ExpandEntry> tab((size_t)in.batch);
    int64_t rows[8] = {};
    const int nrun = f.nrun = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(StagePool::get().helpers() + 1, (int64_t)(p.image.bytes / ((size_t)512 << 10))), in.batch));
    StagePool::get().run(nrun, [&](int k) {
        const int64_t b0 = in.batch * k / nrun, b1 = in.batch * (k + 1) / nrun;
        size_t o = (size_t)b0 * wbytes;
        for (int64_t b = b0; b < b1; ++b) {
            const uint8_t *w = (const uint8_t *)in.x + (size_t)b * wbytes;
            int32_t first, count;
            occupied_run(w, m->depth, row_bytes, &first, &count);
            tab[(size_t)b] = ExpandEntry{(int64_t)o, first, count};
            memcpy((char *)sl.pin_x + o, w + (size_t)first * row_bytes, (size_t)count * row_bytes);
            o += (size_t)count * row_bytes, rows[k] += count;
        }
        f.run[k] = Filled::Run{(size_t)b0 * wbytes, o - (size_t)b0 * wbytes};
    });
    for (int k = 0; k < nrun; ++k) f.rows_shipped += rows[k];
    if (nrun == 1) {  // the layout of these rows handed over
        RingInput found = in;
        found.kind = InKind::Rows, found.rows_total = rows[0];
        p = plan_batch(m, found, false, p.verify.bytes != 0, p.layers.bytes != 0);
    }
    memcpy((char *)sl.pin_x + p.rows_tab.off, tab.data(), p.rows_tab.bytes);
}

// ---- queue the input.  Windows of up to kKernelCopyMax bytes come in through the copy kernel only while no other batch of this handle is
// in flight: behind a running batch the transfer stream brings the windows in under its kernels (pileup ring 4.22 M -> 4.37 M windows/s),
// alone the copy kernel is the shorter way (blocking call of one chunk 3.87 M against 3.64 M)
static int transfer_input(const HostSlot &sl, const StagedBatch &p, const Filled &f, hipStream_t st) {
    if (f.src) TRY(stage_h2d(sl.dev_x, sl.pin_x, f.src, p.image.bytes, st));
    for (int k = 0; k < f.nrun; ++k)
        if (f.run[k].bytes)
            HIP_TRY(hipMemcpyAsync((char *)sl.dev_x + f.run[k].off, (char *)sl.pin_x + f.run[k].off, f.run[k].bytes, hipMemcpyHostToDevice, st));
    if (p.staged > p.tail) HIP_TRY(hipMemcpyAsync((char *)sl.dev_x + p.tail, (char *)sl.pin_x + p.tail, p.staged - p.tail, hipMemcpyHostToDevice, st));
    return 0;
}
static int queue_input(c3_model *m, const HostSlot &sl, const StagedBatch &p, const Filled &f, bool alone, bool in_lane) {
    hipStream_t s = lane(m).stream;
    if (alone && p.staged <= kKernelCopyMax && p.y_total <= kKernelCopyMax && f.nrun <= 1) {  // (the copy kernel moves ONE run: rows packed by several ranges take the transfers)
        if (f.src) StagePool::get().copy(sl.pin_x, f.src, p.image.bytes);  // (plain memcpy below 1 MB, split over the helpers above)
        const size_t from = f.no_image ? p.tail : 0;  // (a section offset: a multiple of 256)
        hipLaunchKernelGGL(host_copy_kernel, dim3(128), dim3(256), 0, s, (const uint4 *)((const char *)sl.pin_x + from), (uint4 *)((char *)sl.dev_x + from),
                           (p.staged - from + 15) / 16, (const uint32_t *)nullptr, (uint32_t *)nullptr);
        HIP_TRY(hipGetLastError());
    } else if (in_lane) {
        // a small batch in a lane brings its windows in on the lane's OWN stream: copy, kernels and the copy-out in order in one queue, no
        // event between two streams -- the batches of the other lanes are what the copy runs under (c3_model.h, the streams)
        TRY(transfer_input(sl, p, f, s));
    } else {
        if (!m->h2d_stream) HIP_TRY(hipStreamCreateWithFlags(&m->h2d_stream, hipStreamNonBlocking));
        TRY(transfer_input(sl, p, f, m->h2d_stream));
        HIP_TRY(hipEventRecord(sl.ev_h2d, m->h2d_stream));
        HIP_TRY(hipStreamWaitEvent(s, sl.ev_h2d, 0));
    }
    return 0;
}

// a candidate batch whose region matrix is on the device already: the image of fill_candidates, laid out by copies between device buffers.
// Queued behind queue_input on the lane's stream (which brings in the tail only: Filled::no_image)
static int queue_device_image(c3_model *m, const HostSlot &sl, const RingInput &in, const StagedBatch &p) {
    const CandInput &ci = *in.cand;
    hipStream_t s = lane(m).stream;
    if (ci.dev_ready) HIP_TRY(hipStreamWaitEvent(s, ci.dev_ready, 0));
    if (!ci.head_tail) {
        if (p.image.bytes) HIP_TRY(hipMemcpyAsync(sl.dev_x, ci.dev_image, p.image.bytes, hipMemcpyDeviceToDevice, s));
        if (ci.dev_taken) HIP_TRY(hipEventRecord(ci.dev_taken, s));
        return 0;
    }
    const size_t colb = (size_t)m->C * sizeof(int32_t), pad = (size_t)(m->positions - 1);
    for (size_t k = 0; k < ci.chunks.size(); ++k) {
        const SelectChunk &ch = ci.chunks[k];
        const size_t n = (size_t)(ch.last - ch.first + 1), c0 = (size_t)ch.col, s0 = (size_t)ci.src_col[k];
        HIP_TRY(hipMemsetAsync((char *)sl.dev_x + (c0 - pad) * colb, 0, pad * colb, s));
        HIP_TRY(hipMemcpyAsync((char *)sl.dev_x + c0 * colb, (const char *)ci.dev_image + s0 * colb, n * colb, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemsetAsync((char *)sl.dev_x + (c0 + n) * colb, 0, pad * colb, s));
    }
    if (ci.dev_taken) HIP_TRY(hipEventRecord(ci.dev_taken, s));
    return 0;
}

// a rows batch whose rows are on the device already: the image of fill_rows by one copy between device buffers.  Queued behind queue_input
// on the lane's stream (which brings in the row table only: Filled::no_image)
static int queue_device_rows(c3_model *m, const HostSlot &sl, const RingInput &in, const StagedBatch &p) {
    hipStream_t s = lane(m).stream;
    if (in.dev_ready) HIP_TRY(hipStreamWaitEvent(s, in.dev_ready, 0));
    if (p.image.bytes) HIP_TRY(hipMemcpyAsync(sl.dev_x, in.dev_rows, p.image.bytes, hipMemcpyDeviceToDevice, s));
    if (in.dev_taken) HIP_TRY(hipEventRecord(in.dev_taken, s));
    return 0;
}

// ---- the exact form on the ring (c3_exact.h, included behind this file): the pass that answers a batch of an exact-answer handle, verify
// mode's second pass against the exact rows, and the repair of C3_VERIFY_REPLACE
static int exact_ring_pass(c3_model *m, hipStream_t s, HostSlot &sl, const StagedBatch &p, int x_dtype, int64_t batch, float *y, double *keep64, bool layers);
static int exact_shadow_pass(c3_model *m, HostSlot &sl, const RingInput &in, const StagedBatch &p);
static int verify_replace_launch(c3_model *m, hipStream_t s, HostSlot &sl, const RingInput &in, const StagedBatch &p, const double *ref64);
// the depths the product and fp32 forms see of a staged batch: none where they were staged for the exact form's gather only (StagedBatch::gather_only)
static const int32_t *ring_depth(const HostSlot &sl, const StagedBatch &p) { return p.gather_only ? nullptr : sl.dev<const int32_t>(p.depth); }

// ---- refine mode (c3_refine.h): the selection behind the product pass, and what c3_predict_wait does with its record
// the two selection launches on stream s over `rows` (row stride `stride`): the windows' minimum gaps, bits and the workgroups' partials into
// `scratch` (RefineScratch(batch).bytes), the record and the ascending list of selected windows into `section`
static int refine_select_launch(hipStream_t s, const float *rows, int stride, int nout, int64_t batch, float gap, void *scratch, void *section) {
    const RefineScratch at(batch);
    RefineGapParams gp;
    gp.rows = rows, gp.min_gap = (float *)scratch, gp.bits = (uint8_t *)scratch + at.bits_at, gp.part = (RefinePart *)((char *)scratch + at.part_at);
    gp.stride = stride, gp.nout = nout, gp.batch = (int)batch, gp.gap = gap;
    const unsigned blocks = refine_blocks(batch);
    hipLaunchKernelGGL(rows_gap_kernel, dim3(blocks), dim3(kRefineThreads), 0, s, gp);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(refine_compact_kernel, dim3(blocks), dim3(64), 0, s, (const uint8_t *)gp.bits, (const RefinePart *)gp.part, (int)batch,
                       (int32_t *)((char *)section + kRefineRecordBytes), (RefineRecord *)section);
    HIP_TRY(hipGetLastError());
    return 0;
}
// which batches the mode covers (c3_model_set_refine in include/c3hip.h lists the ones it does not: they count as skipped)
static bool refine_covers(const c3_model *m, const RingInput &in) {
    return m->refine_on && in.batch > 0 && in.batch <= kRefineMaxBatch && (in.kind == InKind::Sliced || in.kind == InKind::Parts) && !in.depth &&
           !in.score && !m->answer_exact;
}
static int run_refine_select(c3_model *m, hipStream_t s, HostSlot &sl, const StagedBatch &p, int64_t batch, const float *rows) {
    const RefineScratch at(batch);
    if (at.bytes > sl.refine_scratch_bytes) {  // (the slot is free: nothing reads the buffer)
        if (sl.refine_scratch) (void)hipFree(sl.refine_scratch);
        sl.refine_scratch = nullptr, sl.refine_scratch_bytes = 0;
        HIP_TRY(hipMalloc(&sl.refine_scratch, at.bytes));
        sl.refine_scratch_bytes = at.bytes;
    }
    ProfScope ps(m, s, m->kind == C3_KIND_PILEUP ? "p.refine" : "fa.refine", 0.0, (double)batch * m->row * 4.0);
    return refine_select_launch(s, rows, m->row, m->nout, batch, m->refine_gap, sl.refine_scratch, (char *)sl.dev_y + p.refine.off);
}
// the second pass over the selected windows of a batch that came home (c3_exact.h, behind exact_pass)
static int refine_pass(c3_model *m, HostSlot &sl, int64_t n_sel);
static void refine_zero(c3_model *m) {
    m->rfstats = c3_refine_stats{};
    for (float &g : m->rfstats.min_gap) g = INFINITY;
}
// c3_predict_wait, a batch submitted while the mode was on: it joins the totals; one with selected windows runs its second pass here, in its
// lane.  The range guard keeps priority: a batch it answered is not refined
static int refine_account(c3_model *m, HostSlot &sl, bool guarded) {
    const StagedBatch &p = sl.plan;
    c3_refine_stats &t = m->rfstats;
    ++t.batches;
    if (!p.refine.bytes || guarded) return ++t.batches_skipped, 0;
    const RefineRecord *r = (const RefineRecord *)((const char *)sl.pin_y + p.refine.off);
    if (r->windows != (uint32_t)sl.batch || r->selected > r->windows)
        return fail("internal: the refine record counts %u of %u windows selected in a batch of %lld", r->selected, r->windows, (long long)sl.batch);
    if (r->selected > 0) {
        TRY(refine_pass(m, sl, r->selected));  // (the record comes home again, with what the scatter kernel counted)
        ++t.batches_refined;
    }
    t.windows += r->windows, t.windows_selected += r->selected, t.windows_changed += r->changed, t.decoder_selected += r->decoder;
    for (int k = 0; k < 4; ++k) t.head_selected[k] += r->head[k], t.min_gap[k] = std::min(t.min_gap[k], r->min_gap[k]);
    float d;
    memcpy(&d, &r->max_diff_bits, sizeof(d));
    t.max_abs_diff = std::max(t.max_abs_diff, d);
    return 0;
}

// ---- verify mode (c3_verify.h): which batches, the second pass, what c3_predict_wait does with the record
// The submits with batch > 0 are numbered; number k is selected when k % every == 0.  A selected batch that cannot be verified counts as skipped.
// verify_select only LOOKS (true: this batch runs the second pass); verify_count numbers the submit once it is in flight, so that a submit
// which failed on the way has moved no counter and checked + skipped stays the number of selected submits that flew
static bool verify_select(const c3_model *m, int64_t batch, bool can, int64_t *ordinal) {
    if (m->verify_every <= 0 || batch <= 0) return false;
    *ordinal = m->vstats.batches_submitted;
    if (*ordinal % m->verify_every != 0) return false;
    // the second pass must not overwrite what keep mode, the taps or the profile record; a handle on the fp32 forms has nothing to compare
    return can && m->f16_ok && !m->keep && !m->tap_mask && !m->prof;
}
static void verify_count(c3_model *m, int64_t batch, bool verified) {
    if (m->verify_every <= 0 || batch <= 0) return;
    if (m->vstats.batches_submitted++ % m->verify_every == 0 && !verified) ++m->vstats.batches_skipped;
}
// the slot's buffer of shadow rows, the compare kernel's partials behind them: allocated on first use, grown on demand (the slot is free: nothing reads it)
static int ensure_shadow(HostSlot &sl, size_t row_bytes) {
    const size_t part = (row_bytes + 255) & ~(size_t)255, bytes = part + (size_t)kVerifyMaxBlocks * sizeof(VerifyRecord);
    if (bytes > sl.shadow_bytes) {
        if (sl.shadow) (void)hipFree(sl.shadow);
        sl.shadow = nullptr, sl.shadow_bytes = 0;
        HIP_TRY(hipMalloc((void **)&sl.shadow, bytes));
        sl.shadow_bytes = bytes;
    }
    sl.shadow_part = part;
    return 0;
}
// ---- layer records (c3_model_set_verify_layers): the layers in network order as tap ids; returns how many
static int verify_layer_ids(const c3_model *m, int ids[kLayerMaxLayers]) {
    if (m->kind == C3_KIND_PILEUP) return ids[0] = kTapLstm1, ids[1] = kTapGx2, ids[2] = kTapLstm2, ids[3] = kTapL4, 4;
    for (int k = 0; k <= kTapL4; ++k) ids[k] = k;
    return kTapL4 + 1;
}
// what a batch with layer records needs before its first launch: the slot's partials (one launch per layer and micro-batch: a batch is
// cut into at most ceil(batch / max_microbatch) of them, c3_model.h ensure_workspace), the channel exponents on the device, a clean count
static int ensure_layers(c3_model *m, HostSlot &sl, int64_t batch) {
    const int stride = (int)((batch + max_microbatch(m) - 1) / max_microbatch(m)) * kLayerMaxBlocks;
    if (stride > sl.layer_part_stride) {
        if (sl.layer_part) (void)hipFree(sl.layer_part);
        sl.layer_part = nullptr, sl.layer_part_stride = 0;
        HIP_TRY(hipMalloc((void **)&sl.layer_part, (size_t)kTapCount * stride * sizeof(LayerRecord)));
        sl.layer_part_stride = stride;
    }
    if (!m->layer_exp_ok && m->kind == C3_KIND_FULL_ALIGNMENT) {
        std::vector<int> e(9 * 256, 0);
        for (int l = 0; l < 9; ++l) {
            if (m->act_exp[l].size() > 256) return fail("internal: %zu channel exponents in layer %d", m->act_exp[l].size(), l);
            std::copy(m->act_exp[l].begin(), m->act_exp[l].end(), e.begin() + l * 256);
        }
        if (!m->layer_exp) HIP_TRY(hipMalloc((void **)&m->layer_exp, e.size() * sizeof(int)));
        TRY(h2d_staged(m->layer_exp, e.data(), e.size() * sizeof(int)));
        m->layer_exp_ok = true;
    }
    sl.layer_kept = sl.layer_planes = 0, sl.layer_dropped = false;
    for (int &n : sl.layer_parts) n = 0;
    return 0;
}
// The batch again on the fp32 forms, same lane and stream, from the same staged input -- the call range_guard_rerun makes, without touching
// `precision`: a region batch gathers again, depths rescale again, rows expand again, a candidate batch reuses its compacted starts (the
// selection does NOT run again).  Then the compare kernels; the record lands in the slot's output buffer.  What c3_model_describe reports
// of the last forward pass stays the product pass's
static int shadow_pass(c3_model *m, HostSlot &sl, const RingInput &in, const StagedBatch &p) {
    hipStream_t s = lane(m).stream;
    TRY(ensure_shadow(sl, p.y.bytes));
    const c3_model::Choices reported = m->choice;
    const bool f16 = m->f16_ok, planes = lane(m).last_planes;
    m->f16_ok = false;
    if (p.layers.bytes) m->layer_pass = 2;  // every layer's compare launch goes behind the launch that wrote it (c3_forward.h layer_tap)
    const int rc = forward_device(m, s, sl.dev_x, in.x_dtype, in.batch, sl.shadow, sl.dev<const int32_t>(p.starts), ring_depth(sl, p),
                                  sl.dev<const ExpandEntry>(p.rows_tab));
    m->f16_ok = f16, lane(m).last_planes = planes, m->choice = reported, m->layer_pass = 0;
    TRY(rc);
    if (p.layers.bytes) {  // one wave per layer: the partials of its launches -> its record
        LayerFinalParams fp;
        int ids[kLayerMaxLayers];
        const int nl = verify_layer_ids(m, ids);
        fp.part = sl.layer_part, fp.kept = m->layer_kept_count, fp.out = (LayerRecord *)((char *)sl.dev_y + p.layers.off);
        fp.batch = (int)in.batch;
        for (int k = 0; k < kLayerMaxLayers; ++k) fp.part_at[k] = fp.n_parts[k] = 0;
        for (int k = 0; k < nl; ++k) fp.part_at[k] = ids[k] * sl.layer_part_stride, fp.n_parts[k] = sl.layer_parts[ids[k]];  // (partials by tap id, records in network order)
        hipLaunchKernelGGL(layer_compare_final_kernel, dim3((unsigned)nl), dim3(64), 0, s, fp);
        HIP_TRY(hipGetLastError());
    }
    CompareParams cp;
    cp.a = in.y_dev ? in.y_dev : sl.dev_y, cp.b = sl.shadow;
    cp.kept = in.kind == InKind::Candidates ? (const uint32_t *)((const char *)sl.dev_y + p.kept.off) : nullptr;
    cp.part = (VerifyRecord *)((char *)sl.shadow + sl.shadow_part);
    cp.stride = m->row, cp.nout = m->nout, cp.batch = (int)in.batch, cp.tol = m->verify_tol, cp.near_tie = m->verify_near_tie;
    const int blocks = (int)std::min<int64_t>(kVerifyMaxBlocks, (in.batch + kVerifyThreads / 4 - 1) / (kVerifyThreads / 4));
    hipLaunchKernelGGL(rows_compare_kernel, dim3((unsigned)blocks), dim3(kVerifyThreads), 0, s, cp);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rows_compare_final_kernel, dim3(1), dim3(64), 0, s, (const VerifyRecord *)cp.part, blocks, cp.kept, (int)in.batch,
                       (VerifyRecord *)((char *)sl.dev_y + p.verify.off));
    HIP_TRY(hipGetLastError());
    if (m->verify_policy == C3_VERIFY_REPLACE) TRY(verify_replace_launch(m, s, sl, in, p, nullptr));
    return 0;
}
// c3_predict_wait, a verified batch the range guard did not answer: the record joins the totals; true = the policy escalates this batch
static bool verify_account(c3_model *m, const HostSlot &sl) {
    const char *rec = (const char *)sl.pin_y + sl.plan.verify.off;
    const VerifyRecord &r = *(const VerifyRecord *)rec;
    c3_verify_stats &t = m->vstats;
    const bool ref_exact = m->verify_ref == C3_VERIFY_REF_EXACT;  // (neither setting changes while a batch is in flight)
    if (ref_exact) {  // the double maximum behind the record (c3_exact.h)
        double d;
        memcpy(&d, rec + kVerifyMax64At, sizeof(d));
        m->vextra.max_abs_diff_f64 = std::max(m->vextra.max_abs_diff_f64, d);
    }
    if (m->verify_policy == C3_VERIFY_REPLACE) {  // ... and the rows repaired on the device
        uint32_t n;
        memcpy(&n, rec + kVerifyReplacedAt, sizeof(n));
        m->vextra.rows_replaced += n, m->vextra.batches_with_replacements += n > 0;
    }
    ++t.batches_checked, t.windows_checked += r.n, t.rows_over_tol += r.rows_over;
    if (t.worst_batch < 0 || r.max_abs > t.max_abs_diff) t.worst_batch = sl.verify_ordinal, t.worst_row = r.worst_row, t.max_abs_diff = r.max_abs;
    int64_t labels = 0;
    for (int k = 0; k < 4; ++k) {
        t.head_max_abs_diff[k] = std::max(t.head_max_abs_diff[k], r.head_max[k]);
        t.label_diffs[k] += r.label[k], t.near_ties[k] += r.tie[k], labels += r.label[k];
    }
    if (m->verify_policy != C3_VERIFY_ESCALATE || (r.rows_over == 0 && labels == 0)) return false;
    ++t.escalations;
    if (m->f16_ok)
        fprintf(stderr, "libc3hip: verify mode: fp16x3 rows differ from the %s (max |d| = %.3g, %u rows beyond %.3g, %lld labels); this handle "
                        "continues on fp32 matrix instructions\n", ref_exact ? "exact form" : "fp32 forms", (double)r.max_abs, r.rows_over, (double)m->verify_tol,
                (long long)labels);
    m->f16_ok = false, m->precision = "fp32-verify";
    return true;
}

// ... and its layer records, when it brought some, join the layers' totals (the rule of worst_batch above, per layer)
static void verify_layers_account(c3_model *m, const HostSlot &sl) {
    if (!sl.plan.layers.bytes) return;
    const LayerRecord *r = (const LayerRecord *)((const char *)sl.pin_y + sl.plan.layers.off);
    int ids[kLayerMaxLayers];
    const int nl = verify_layer_ids(m, ids);
    bool any = false;
    for (int k = 0; k < nl; ++k) any |= r[k].compared != 0;
    if (!any) return;  // (the slot had no room for the layer outputs: c3_forward.h layer_tap)
    ++m->vlayer_batches;
    for (int k = 0; k < nl; ++k) {
        if (!r[k].compared) continue;
        c3_verify_layer &t = m->vlayer[k];
        ++t.batches, t.windows += r[k].windows;
        if (t.worst_batch < 0 || r[k].max_abs > t.max_abs_diff)
            t.worst_batch = sl.verify_ordinal, t.worst_window = r[k].window, t.worst_index = r[k].index, t.max_abs_diff = r[k].max_abs;
        t.ref_max_abs = std::max(t.ref_max_abs, r[k].ref_max), t.test_max_abs = std::max(t.test_max_abs, r[k].test_max);
    }
}

// ---- score mode (c3_score.h): the two launches on stream s over `rows` (row stride m->row) and the labels staged with the batch; the record
// -- and the windows' values when the plan has room for them -- land in the slot's output buffer
static int score_launch(c3_model *m, hipStream_t s, const float *rows, int stride, const void *labels, int label_dtype, int64_t batch, float *loss,
                        uint64_t *part, ScoreRecord *out) {
    ScoreParams sp;
    sp.rows = rows, sp.labels = labels, sp.loss = loss, sp.part = part, sp.gamma = m->score_gamma;
    sp.stride = stride, sp.nout = m->nout, sp.tasks = m->nb, sp.batch = (int)batch;
    sp.label_f32 = label_dtype == C3_DTYPE_F32, sp.weighted = m->score_weighted;
    memcpy(sp.w, m->score_w, sizeof(sp.w));
    const int blocks = score_blocks(batch);
    ProfScope ps(m, s, m->kind == C3_KIND_PILEUP ? "p.score" : "fa.score", 0.0, (double)batch * m->nout * (4.0 + (sp.label_f32 ? 4.0 : 1.0)));
    hipLaunchKernelGGL(rows_score_kernel, dim3((unsigned)blocks), dim3(kScoreThreads), 0, s, sp);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rows_score_final_kernel, dim3(1), dim3(64), 0, s, (const uint64_t *)part, blocks, (int)batch, m->nb, out);
    HIP_TRY(hipGetLastError());
    return 0;
}
static int run_score(c3_model *m, hipStream_t s, HostSlot &sl, const StagedBatch &p, int label_dtype, int64_t batch, const float *rows) {
    if (!sl.score_part) HIP_TRY(hipMalloc((void **)&sl.score_part, kScorePartBytes));
    return score_launch(m, s, rows, m->row, sl.dev<const char>(p.labels), label_dtype, batch, p.losses.bytes ? (float *)((char *)sl.dev_y + p.losses.off) : nullptr,
                        sl.score_part, (ScoreRecord *)((char *)sl.dev_y + p.score.off));
}
// ---- the census of score mode (c3_census.h): the batch's table is zeroed and filled on stream s, behind the score kernels and from the same
// rows and labels; a re-run rewrites it, so nothing accumulates on the device
static int census_launch(c3_model *m, hipStream_t s, const float *rows, int stride, const void *labels, int label_dtype, int64_t batch,
                         ScoreCensusTable *out) {
    ScoreCensusParams cp;
    cp.rows = rows, cp.labels = labels, cp.out = out;
    cp.stride = stride, cp.nout = m->nout, cp.batch = (int)batch, cp.label_f32 = label_dtype == C3_DTYPE_F32;
    ProfScope ps(m, s, m->kind == C3_KIND_PILEUP ? "p.census" : "fa.census", 0.0, (double)batch * m->nout * (4.0 + (cp.label_f32 ? 4.0 : 1.0)));
    HIP_TRY(hipMemsetAsync(out, 0, sizeof(ScoreCensusTable), s));
    hipLaunchKernelGGL(rows_census_kernel, dim3((unsigned)score_census_blocks(batch)), dim3(kScoreCensusThreads), 0, s, cp);
    HIP_TRY(hipGetLastError());
    return 0;
}
static int run_census(c3_model *m, hipStream_t s, HostSlot &sl, const StagedBatch &p, int label_dtype, int64_t batch, const float *rows) {
    return census_launch(m, s, rows, m->row, sl.dev<const char>(p.labels), label_dtype, batch, (ScoreCensusTable *)((char *)sl.dev_y + p.census.off));
}
// one completed batch of `windows` windows joins the handle's totals: 32-bit counts widened here
static void census_add(c3_score_census &total, const ScoreCensusTable &t, int64_t windows, int tasks) {
    total.windows += windows, total.tasks = tasks;
    for (int i = 0; i < kScoreCensusCells; ++i) total.confusion[i] += t.confusion[i];
    for (int h = 0; h < 4; ++h) {
        for (int b = 0; b < kScoreCensusBins; ++b) {
            total.rel_windows[h][b] += t.rel_windows[h][b], total.rel_correct[h][b] += t.rel_correct[h][b];
            total.rel_conf_q32[h][b] += (int64_t)t.rel_conf_q32[h][b];
        }
        total.rel_skipped[h] += t.rel_skipped[h];
        for (int k = 0; k < kScoreCensusGaps; ++k) total.gap_below[h][k] += t.gap_below[h][k];
    }
}
// c3_predict_wait's reader of a scored batch: the record out of the pinned output buffer, the windows' values to where the caller wants them,
// the batch's census table into the handle's totals -- once per completed batch, whoever waits for it
static void read_score(HostSlot &sl, c3_model *m = nullptr) {
    const StagedBatch &p = sl.plan;
    memcpy(&sl.score_rec, (const char *)sl.pin_y + p.score.off, sizeof(ScoreRecord));
    if (sl.loss_host && p.losses.bytes) memcpy(sl.loss_host, (const char *)sl.pin_y + p.losses.off, p.losses.bytes);
    if (m && p.census.bytes) {
        ScoreCensusTable t;
        memcpy(&t, (const char *)sl.pin_y + p.census.off, sizeof(t));
        census_add(m->score_census, t, sl.batch, m->nb);
    }
}
// c3_predict_wait, a scored batch that another pass answered in the end (the range guard's re-run under either policy, verify mode's
// escalation): scored again on the rows it is answered with, from the labels still staged; the record and the values come over again
static int rescore(c3_model *m, HostSlot &sl, const float *rows) {
    const StagedBatch &p = sl.plan;
    TRY(use_lane(m, sl.lane));
    hipStream_t s = lane(m).stream;
    TRY(run_score(m, s, sl, p, sl.label_dtype, sl.batch, rows));
    if (p.census.bytes) TRY(run_census(m, s, sl, p, sl.label_dtype, sl.batch, rows));
    HIP_TRY(hipMemcpyAsync((char *)sl.pin_y + p.score.off, (const char *)sl.dev_y + p.score.off, p.y_total - p.score.off, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

// ---- launch, on the active lane's stream: the selection in front of a candidate batch, the forward pass, the rows on their way out
static int launch_batch(c3_model *m, HostSlot &sl, const RingInput &in, const StagedBatch &p) {
    hipStream_t s = lane(m).stream;
    if (in.kind == InKind::Candidates) {
        SelectParams sp;
        sp.x = (const int32_t *)sl.dev_x, sp.chunks = sl.dev<const SelectChunk>(p.chunks);
        sp.pos = sl.dev<const int64_t>(p.cand_pos), sp.depth_in = sl.dev<const int32_t>(p.depth_in);
        sp.status = (uint8_t *)sl.dev_y + p.status.off, sp.start_all = sl.dev<int32_t>(p.start_all), sp.starts = sl.dev<int32_t>(p.starts);
        sp.depth = sl.dev<int32_t>(p.depth), sp.block_kept = sl.dev<uint32_t>(p.tiles), sp.n_rows = (uint32_t *)((char *)sl.dev_y + p.kept.off);
        sp.n_cand = (int)in.batch, sp.n_chunks = (int)in.cand->chunks.size(), sp.C = m->C, sp.T = m->positions, sp.head_tail = in.cand->head_tail;
        sp.img_cols = in.n_cols;
        TRY(run_select(m, s, sp));
    }
    const bool exact = m->answer_exact;  // the batch is answered by the exact form (c3_exact.h): no product kernel, the range flag neither raised nor read
    const bool f16 = m->f16_ok && !exact;
    if (p.layers.bytes) {  // layer records: the product pass keeps its layer outputs in the slot (c3_forward.h layer_tap)
        TRY(ensure_layers(m, sl, in.batch));
        m->layer_slot = &sl, m->layer_batch = in.batch, m->layer_pass = 1;
        m->layer_kept_count = in.kind == InKind::Candidates ? (const uint32_t *)((const char *)sl.dev_y + p.kept.off) : nullptr;
    }
    const int rc_product = exact ? exact_ring_pass(m, s, sl, p, in.x_dtype, in.batch, in.y_dev ? in.y_dev : sl.dev_y, nullptr, false)
                                 : forward_device(m, s, sl.dev_x, in.x_dtype, in.batch, in.y_dev ? in.y_dev : sl.dev_y, sl.dev<const int32_t>(p.starts),
                                                  ring_depth(sl, p), sl.dev<const ExpandEntry>(p.rows_tab));
    m->layer_pass = 0;
    TRY(rc_product);
    if (in.y_dev && f16)  // rows that stay on the device are scanned there (bit 1 of the flag: a non-finite row)
        hipLaunchKernelGGL(rows_finite_kernel, dim3((unsigned)((in.batch * m->row + 255) / 256)), dim3(256), 0, s, in.y_dev, in.batch * m->row, m->range_flag);
    const bool rows_home = in.score && !in.y_host;  // (a scored batch whose caller wants no rows: scanned here like rows that stay on the device)
    if (rows_home && f16)
        hipLaunchKernelGGL(rows_finite_kernel, dim3((unsigned)((in.batch * m->row + 255) / 256)), dim3(256), 0, s, sl.dev_y, in.batch * m->row, m->range_flag);
    if (p.verify.bytes) TRY(m->verify_ref == C3_VERIFY_REF_EXACT ? exact_shadow_pass(m, sl, in, p) : shadow_pass(m, sl, in, p));
    if (p.score.bytes) TRY(run_score(m, s, sl, p, in.label_dtype, in.batch, sl.dev_y));
    if (p.census.bytes) TRY(run_census(m, s, sl, p, in.label_dtype, in.batch, sl.dev_y));
    if (p.refine.bytes) TRY(run_refine_select(m, s, sl, p, in.batch, in.y_dev ? in.y_dev : sl.dev_y));
    // the rows (96 - 484 B per window) and the range flag leave through a copy kernel on the COMPUTE stream, whatever the
    // batch: handing them to a transfer stream (event, cross-queue wait, two DMA copies, event) cost the compute queue
    // ~75 us per batch -- 538 k -> 647 k windows/s host to host at B = 256 (profiles/r03_e_d2h_by_kernel.txt)
    if (rows_home) {  // only the records (a verified batch: from its verify record on) and the windows' values leave
        const size_t from = p.verify.bytes ? p.verify.off : p.score.off;
        hipLaunchKernelGGL(host_copy_kernel, dim3(rows_out_grid(p.y_total - from)), dim3(256), 0, s, (const uint4 *)((const char *)sl.dev_y + from),
                           (uint4 *)((char *)sl.pin_y + from), (p.y_total - from + 15) / 16, (const uint32_t *)m->range_flag, sl.pin_flag);
    } else
        hipLaunchKernelGGL(host_copy_kernel, dim3(in.y_dev ? 1 : rows_out_grid(p.y_total)), dim3(256), 0, s, (const uint4 *)sl.dev_y, (uint4 *)sl.pin_y,
                           in.y_dev ? (p.verify.bytes + p.layers.bytes + p.refine.bytes) / 16 : (p.y_total + 15) / 16, (const uint32_t *)m->range_flag, sl.pin_flag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(sl.ev_out, s));
    sl.used_f16 = f16;
    return 0;
}

// ---- record: the slot becomes busy, with everything c3_predict_wait needs (launched: false -- a candidate batch with nothing to launch)
static void record_batch(const c3_model *m, HostSlot &sl, const RingInput &in, const StagedBatch &p, int64_t rows_shipped, bool launched = true) {
    sl.plan = p, sl.batch = in.batch, sl.x_dtype = in.x_dtype, sl.y_host = in.y_host, sl.y_dev_out = in.y_dev;
    sl.lane = m->lane_cur, sl.tap_off = m->tap_call_off, sl.rows_shipped = rows_shipped;
    sl.cand = in.cand != nullptr, sl.cand_none = !launched;
    sl.verified = p.verify.bytes != 0;
    if (in.cand) sl.status_host = in.cand->status_host, sl.n_rows_host = in.cand->n_rows_host, sl.n_chunks = (int64_t)in.cand->chunks.size();
    sl.n_parts = in.kind == InKind::Parts ? in.n_parts : 0;
    for (int i = 0; i < sl.n_parts; ++i) sl.part_count[i] = in.counts[i], sl.part_y[i] = in.y_parts[i];
    sl.pack_epoch = m->pack_epoch;
    sl.scored = in.score, sl.rows_home = in.score && !in.y_host, sl.label_dtype = in.label_dtype, sl.loss_host = in.loss_host;
    sl.score_rec = ScoreRecord{}, sl.score_rec.tasks = m->nb;  // (a batch of no windows: what c3_score_wait reports)
    sl.refine_on = m->refine_on;
    sl.busy = true;
}

static int predict_submit(c3_model *m, RingInput in, int slot) {
    TRY(ring_ready(m, slot));
    if (in.batch < 0) return fail("negative batch");
    if (in.kind != InKind::Parts && in.batch > 0 && (!in.x || (!in.y_host && !in.y_dev && !in.score))) return fail("null buffer");  // (parts: checked one by one at the entry)
    // the exact form gathers the windows of a region with the int32 pre-pass of c3_rescale.h: an int8 region matrix cannot be read by it
    const bool region_kind = in.kind == InKind::Region || in.kind == InKind::Candidates, exact_can = !(region_kind && in.x_dtype == C3_DTYPE_I8);
    if (m->answer_exact && !exact_can)
        return fail("the exact form is refused for an int8 region matrix: its windows are gathered by the int32 pre-pass -- pass int32 / int64 counts, or sliced windows");
    HIP_TRY(hipSetDevice(m->device));
    if (in.kind == InKind::Sliced && m->pack_rows && m->kind == C3_KIND_FULL_ALIGNMENT && in.x_dtype == C3_DTYPE_I8 && !in.score) in.kind = InKind::PackedHere;  // (a scored batch stays sliced)
    HostSlot &sl = m->slot[slot];
    // A small batch runs in the next lane (c3_model.h Lane): its own workspace and kernel stream, so that it overlaps the batches before it
    // on the chip; keep mode and profiling stay in one lane -- and so does a batch that fills the chip by itself: two of those side by side
    // only get in each other's way (same-box A/B, profiles/r06_i_ab_ring_lanes.txt: full alignment ring +5.5 % at B = 256, -4 % at B = 1000).
    // Lanes are dealt in the ORDER of the submits, not by slot number: three slots on two lanes (the pileup network) would put two of every
    // three batches behind each other in lane 0 (profiles/r06_n_ab_lane_sharing.txt)
    const bool in_lane = m->ring_lanes > 1 && in.batch <= m->lane_max_batch && !m->keep && !m->prof;
    TRY(use_lane(m, in_lane ? (int)(m->lane_next++ % (unsigned)m->ring_lanes) : 0));
    bool alone = true;
    for (int k = 0; k < kHostSlots; ++k) alone &= !m->slot[k].busy;
    const LaneSharing shared_chip_forms(m, in.batch, in_lane && !alone);
    const int32_t *depth = deep_depths(m, in);
    // (an exact-answer batch is skipped like a batch of a handle on the fp32 forms; so is a batch the exact reference cannot read)
    const bool verify = verify_select(m, in.batch, !m->answer_exact && (m->verify_ref != C3_VERIFY_REF_EXACT || exact_can), &sl.verify_ordinal);
    // a region / candidate batch the exact form reads always stages depths -- the caller's, or zeros: the pre-pass then is the plain gather
    std::vector<int32_t> no_depth;
    bool gather_only = false;
    if (region_kind && !depth && in.batch > 0 && (m->answer_exact || (verify && m->verify_ref == C3_VERIFY_REF_EXACT))) {
        if (!in.depth) no_depth.assign((size_t)in.batch, 0);
        depth = in.depth ? in.depth : no_depth.data(), gather_only = true;
    }
    StagedBatch p = plan_batch(m, in, depth != nullptr, verify, m->verify_layers, refine_covers(m, in));
    p.gather_only = gather_only;
    Filled f;
    if (in.batch > 0) {
        // the slot becomes busy only once everything has been queued: a failure on the way leaves it free
        TRY(ensure_slot(sl, p.x_cap, in.y_dev ? p.verify.bytes + p.layers.bytes + p.refine.bytes : p.y_total));  // (rows that stay on the device need no slot buffers)
        switch (in.kind) {
        case InKind::Sliced: fill_sliced(sl, in, p, depth, f), fill_labels(sl, in, p); break;
        case InKind::Region: fill_region(m, sl, in, p, depth, f); break;
        case InKind::Candidates: fill_candidates(m, sl, in, p, depth, f); break;
        case InKind::Rows: fill_rows(m, sl, in, p, f); break;
        case InKind::PackedHere: fill_packed_rows(m, sl, in, p, f); break;
        case InKind::Parts: fill_parts(sl, in, p, (size_t)c3_model_window_bytes(m, in.x_dtype), f); break;
        }
        TRY(queue_input(m, sl, p, f, alone, in_lane));
        if (in.cand && in.cand->dev_image) TRY(queue_device_image(m, sl, in, p));
        if (in.dev_rows) TRY(queue_device_rows(m, sl, in, p));
        if (launch_batch(m, sl, in, p) != 0) {
            // refused behind its input: the slot stays free, so the next submit may stage into it at once, in ANOTHER lane's stream -- the
            // transfers queued above must have landed before that (the error message is the launch's)
            const std::string why = g_err;
            (void)hipStreamSynchronize(lane(m).stream);
            if (m->h2d_stream) (void)hipStreamSynchronize(m->h2d_stream);
            g_err = why;
            return 1;
        }
    }
    verify_count(m, in.batch, verify);
    record_batch(m, sl, in, p, is_rows(in.kind) ? f.rows_shipped : -1);
    return 0;
}

int c3_predict_submit(c3_model *m, const void *x_host, int x_dtype, int64_t batch, float *y_host, int slot) {
    return predict_submit(m, ring_input(InKind::Sliced, x_host, x_dtype, batch, y_host), slot);
}
// the ring with the rows LEFT ON THE DEVICE (a rank of a sharded job: its rows go to the RCCL gather, not to this host): the
// forward pass writes them straight into the caller's device buffer, only the range flag crosses PCIe
int c3_predict_submit_dev(c3_model *m, const void *x_host, int x_dtype, int64_t batch, float *y_dev, int slot) {
    if (batch > 0 && !y_dev) return fail("null device buffer");
    return predict_submit(m, ring_input(InKind::Sliced, x_host, x_dtype, batch, nullptr, nullptr, y_dev), slot);
}

// ------------------------------------------------------------------------------------------ the range guard
// Safety net of the fp16x3 products: an activation beyond the fp16 range (|x| >= 65504; never seen) surfaces as inf / NaN
// rows or as the range flag (sticky: an overflow in any earlier fp16x3 batch also lands here, which only costs a re-run).  This handle
// continues on fp32 matrix instructions, and the batch runs again on stream s (tap_off: its first window in a c3_predict call of pieces)
static int range_guard_rerun(c3_model *m, hipStream_t s, const void *x_dev, int x_dtype, int64_t batch, float *y_dev, int64_t tap_off = 0,
                             const int32_t *starts = nullptr, const int32_t *depth = nullptr, const ExpandEntry *rows = nullptr) {
    if (m->f16_ok)
        fprintf(stderr, "libc3hip: activations beyond the range of the fp16x3 kernels; this handle continues on fp32 matrix instructions\n");
    m->f16_ok = false, m->precision = "fp32-range-guard";
    m->tap_call_off = tap_off;
    const int rc = forward_device(m, s, x_dev, x_dtype, batch, y_dev, starts, depth, rows);
    m->tap_call_off = 0;
    return rc;
}
// ---- the policy C3_RANGE_RECALIBRATE (c3_calibrate.h, included behind this file): a trip recalibrates instead
static int range_guard_recalibrate(c3_model *m, hipStream_t s, const void *x_dev, int x_dtype, int64_t batch, float *y_dev, int64_t tap_off = 0,
                                   const int32_t *starts = nullptr, const int32_t *depth = nullptr, const ExpandEntry *rows = nullptr);
static bool range_recalibrates(const c3_model *m) {
    // (kept: a load that failed half way left none -- the weights on the device are then not the ones a repack would pack from)
    return m->range_policy == C3_RANGE_RECALIBRATE && m->range_max_recal > 0 && !m->rstats.fell_back && m->f16_ok && !m->kept.empty();
}
// what c3_predict_wait reads of a batch the fp16x3 kernels computed: its copy of the range flag, and its rows where they came to this host
static bool slot_out_of_range(const HostSlot &sl) {
    bool bad = *sl.pin_flag != 0;  // a conv stage produced a value near the fp16 range (kF16Range), or the device scan found a non-finite row
    if (!sl.y_dev_out && !sl.rows_home) {
        const uint32_t *u = reinterpret_cast<const uint32_t *>(sl.pin_y);
        for (size_t i = 0, n = sl.plan.y.bytes / 4; i < n; ++i) bad |= (u[i] & 0x7f800000u) == 0x7f800000u;
    }
    return bad;
}
// A batch that was in flight across a recalibration (its packing is older than the handle's) and came back with its flag copy raised -- the
// flag word is sticky, so that is every such batch -- or with a non-finite row: again on the PRODUCT forms with the weights as they are packed
// now, in its lane, from what was staged; then it is read like a fresh batch (*bad: it tripped again)
static int range_guard_stale_rerun(c3_model *m, HostSlot &sl, bool *bad) {
    const StagedBatch &p = sl.plan;
    TRY(use_lane(m, sl.lane));
    hipStream_t s = lane(m).stream;
    float *y = sl.y_dev_out ? sl.y_dev_out : sl.dev_y;
    m->tap_call_off = sl.tap_off;
    const int rc = forward_device(m, s, sl.dev_x, sl.x_dtype, sl.batch, y, sl.dev<const int32_t>(p.starts), ring_depth(sl, p),
                                  sl.dev<const ExpandEntry>(p.rows_tab));
    m->tap_call_off = 0;
    TRY(rc);
    if (sl.y_dev_out || sl.rows_home) {
        hipLaunchKernelGGL(rows_finite_kernel, dim3((unsigned)((sl.batch * m->row + 255) / 256)), dim3(256), 0, s, y, sl.batch * m->row, m->range_flag);
        HIP_TRY(hipGetLastError());
    } else HIP_TRY(hipMemcpyAsync(sl.pin_y, sl.dev_y, p.y.bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(sl.pin_flag, m->range_flag, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    sl.pack_epoch = m->pack_epoch, ++m->rstats.reruns;
    *bad = slot_out_of_range(sl);
    return 0;
}
int c3_predict_wait(c3_model *m, int slot) {
    TRY(ring_ready(m, slot, false));
    HostSlot &sl = m->slot[slot];
    if (!sl.busy) return fail("slot %d has nothing in flight", slot);
    sl.busy = false;
    const StagedBatch &p = sl.plan;
    // windows that travelled as occupied rows in the call this completes, and their rows (c3_model_describe)
    if (!m->rows_call) m->rows_windows = m->rows_shipped = 0;
    if (sl.rows_shipped >= 0) m->rows_windows += sl.batch, m->rows_shipped += sl.rows_shipped;
    if (sl.cand && sl.cand_none) {  // nothing was launched: no candidate has a window
        if (sl.batch > 0) memset(sl.status_host, kCandNoWindow, (size_t)sl.batch);
        *sl.n_rows_host = 0;
        m->cand_n = sl.batch, m->cand_kept = 0, m->cand_chunks = sl.n_chunks, m->rescaled = 0;
        sl.cand = false;
        return 0;
    }
    if (p.y.bytes == 0) return 0;
    HIP_TRY(hipEventSynchronize(sl.ev_out));
    // per batch: what matters is how THIS slot's rows were computed, not what the handle does now (another slot's wait may have switched it
    // to fp32 while this batch was in flight).  Rows that stayed on the device were scanned there: the flag is all there is to read
    const bool guarded = sl.used_f16 && slot_out_of_range(sl);
    bool bad = guarded;
    if (bad && range_recalibrates(m) && sl.pack_epoch != m->pack_epoch) TRY(range_guard_stale_rerun(m, sl, &bad));
    if (bad) {  // in the batch's lane, from what was staged (a region batch gathers again, a batch with depths rescales again, a rows batch expands again: nothing has written dev_x)
        TRY(use_lane(m, sl.lane));
        const auto rerun = range_recalibrates(m) ? range_guard_recalibrate : range_guard_rerun;
        TRY(rerun(m, lane(m).stream, sl.dev_x, sl.x_dtype, sl.batch, sl.y_dev_out ? sl.y_dev_out : sl.dev_y, sl.tap_off,
                  sl.dev<const int32_t>(p.starts), ring_depth(sl, p), sl.dev<const ExpandEntry>(p.rows_tab)));
        if (!sl.y_dev_out && !sl.rows_home) HIP_TRY(hipMemcpyAsync(sl.pin_y, sl.dev_y, p.y.bytes, hipMemcpyDeviceToHost, lane(m).stream));
        HIP_TRY(hipStreamSynchronize(lane(m).stream));
    }
    const float *answered = guarded ? sl.dev_y : nullptr;  // a scored batch: the rows of the pass that answers it, where another pass than the first does
    if (sl.verified) {  // the range guard keeps priority: a batch it answered counts as skipped
        if (!guarded) verify_layers_account(m, sl);
        if (guarded) ++m->vstats.batches_skipped;
        else if (verify_account(m, sl)) {  // escalate: the batch is answered with its rows on the fp32 forms, decoder columns included
            TRY(use_lane(m, sl.lane));
            if (sl.y_dev_out) HIP_TRY(hipMemcpyAsync(sl.y_dev_out, sl.shadow, p.y.bytes, hipMemcpyDeviceToDevice, lane(m).stream));
            else if (!sl.rows_home) HIP_TRY(hipMemcpyAsync(sl.pin_y, sl.shadow, p.y.bytes, hipMemcpyDeviceToHost, lane(m).stream));
            HIP_TRY(hipStreamSynchronize(lane(m).stream));
            answered = sl.shadow;
        }
    }
    if (sl.refine_on) TRY(refine_account(m, sl, guarded));  // refine mode (c3_refine.h): the windows near a tie are answered by the exact form
    if (sl.scored) {  // the record and the windows' values, of the rows the batch is answered with
        if (answered) TRY(rescore(m, sl, answered));
        read_score(sl, m);
        if (sl.rows_home) return 0;
    }
    if (sl.y_dev_out) return 0;
    if (sl.cand) {  // rows [0, kept) are the result; the rest belong to the surplus windows of dropped candidates
        const int64_t kept = (int64_t)*(const uint32_t *)((const char *)sl.pin_y + p.kept.off);
        if (kept < 0 || kept > sl.batch) return fail("internal: %lld of %lld candidates kept", (long long)kept, (long long)sl.batch);
        memcpy(sl.status_host, (const char *)sl.pin_y + p.status.off, (size_t)sl.batch);
        memcpy(sl.y_host, sl.pin_y, (size_t)kept * m->row * sizeof(float));
        *sl.n_rows_host = kept;
        // the count of rescaled windows among the kept, from the candidates' depths as staged (c3_model_describe)
        int64_t deep = 0;
        if (const int32_t *d = sl.pin<const int32_t>(p.depth_in))
            for (int64_t i = 0; i < sl.batch; ++i) {
                const uint8_t st = sl.status_host[i];
                deep += (st == kCandMain || st == kCandHead || st == kCandTail) && d[i] > 0 && (double)d[i] > 1.5 * (double)m->max_depth;
            }
        m->cand_n = sl.batch, m->cand_kept = kept, m->cand_chunks = sl.n_chunks, m->rescaled = deep;
        sl.cand = false;
        return 0;
    }
    if (sl.n_parts) scatter_parts(sl, (size_t)m->row * sizeof(float));  // (whoever wrote pin_y: the product pass, the range guard's re-run, verify mode's escalation)
    else memcpy(sl.y_host, sl.pin_y, p.y.bytes);
    return 0;
}

// The synchronous call of the reference loop (_torch_predict: H2D, forward, D2H one after the other,
// clair3/CallVariantsFromCffi.py:48-52).  A batch well beyond one chunk (256 full-alignment / 4096 pileup windows; env
// C3HIP_PREDICT_CHUNK) is cut into chunks that travel through the submit / wait ring: the staging copy and H2D transfer of chunk
// i + 1 and the D2H transfer of chunk i - 1 run under the kernels of chunk i, so the caller's ONE blocking call costs little more
// than the kernels of the whole batch.  Rows do not depend on the cut (a window's row is independent of the batch it travels in).
static int64_t predict_chunk(const c3_model *m) {
    static const int64_t env = getenv("C3HIP_PREDICT_CHUNK") ? atoll(getenv("C3HIP_PREDICT_CHUNK")) : -1;
    if (env >= 0) return env;  // 0: never cut
    return m->kind == C3_KIND_PILEUP ? 4096 : 256;
}

static int predict_blocking(c3_model *m, const void *x_host, int x_dtype, int64_t batch, const int32_t *depth_host, float *y_host) {
    if (!m) return fail("null model");
    const int64_t chunk = predict_chunk(m);
    RingInput in = ring_input(InKind::Sliced, x_host, x_dtype, batch, y_host, depth_host);
    if (chunk <= 0 || batch < 2 * chunk) {
        TRY(predict_submit(m, in, 0));
        return c3_predict_wait(m, 0);
    }
    m->rescaled = 0, in.piece = true;
    constexpr int kRing = 3;
    const int64_t wbytes = c3_model_window_bytes(m, x_dtype);
    // A blocking call cannot hide its FIRST staging copy behind a previous batch (pageable -> pinned, ~16 GB/s with the staging pool);
    // every later piece's copy and transfer run under the kernels of the piece before it.
    int64_t n_sub = 0, n_done = 0;  // chunks submitted / waited for
    int rc = 0;
    // piece sizes grow threefold from a quarter of the batch (between chunk / 2 and chunk): the kernels start after a SHORT first
    // transfer, every later transfer hides under the kernels of the piece before it (a full-alignment window takes 0.42 us to
    // cross PCIe and 1.3 us to compute), and few big pieces fill the chip better than many small ones -- 1000 windows as 250 +
    // 750 instead of 128 + 256 + 616: 0.79 -> 0.82 of device-resident; a tail shorter than half the next size joins the last piece
    int64_t next = std::min<int64_t>(std::max<int64_t>(chunk / 2, batch / 4), chunk);
    next = std::max<int64_t>(next, 1);
    // A batch that fits the ring's lanes as EQUAL pieces -- one lane-sized piece per lane: 334 + 333 + 333 full-alignment windows for the
    // reference's batch of 1000 -- is cut that way: every piece brings its windows in on its own lane's stream and runs beside the others
    // (profiles/r06_o_*: 656 - 667 k -> 700 - 721 k windows/s same-box against the growing pieces; with the lanes' first form -- up to three
    // streams each -- the same cut LOST 4 %, profiles/r06_i_ab_ring_lanes.txt, r06_j_blocking_call_pieces.txt).
    const bool lanes_on = m->ring_lanes > 1 && !m->keep && !m->prof;
    const int64_t equal = (lanes_on && m->kind == C3_KIND_FULL_ALIGNMENT && batch <= (int64_t)m->ring_lanes * m->lane_max_batch)
                              ? (batch + m->ring_lanes - 1) / m->ring_lanes : 0;
    // debug taps (c3_debug_tap): every piece's windows at their place in this call
    if (m->tap_mask) {
        TRY(tap_prepare(m, batch));
        m->tap_call = true;
    }
    m->rows_windows = m->rows_shipped = 0, m->rows_call = true;  // (C3HIP_PACK_ROWS=1: the pieces' counts add up)
    for (int64_t off = 0; off < batch && rc == 0; ++n_sub) {
        int64_t take = std::min(next, batch - off);
        if (batch - off - take < next / 2 || batch - off - take < chunk / 2) take = batch - off;
        if (equal > 0) take = std::min(equal, batch - off);
        take = std::min(take, max_microbatch(m));
        if (n_sub - n_done == kRing) rc = c3_predict_wait(m, (int)(n_done++ % kRing));
        m->tap_call_off = off;
        in.x = (const char *)x_host + off * wbytes, in.batch = take, in.y_host = y_host + off * m->row;
        if (depth_host) in.depth = depth_host + off;
        if (rc == 0) rc = predict_submit(m, in, (int)(n_sub % kRing));
        m->tap_call_off = 0;
        if (rc != 0) break;
        off += take;
        next = std::min(3 * next, 4 * chunk);
    }
    const std::string first_error = rc != 0 ? g_err : std::string();
    for (; n_done < n_sub; ++n_done) {  // drain, also after an error: no slot stays busy behind a failed call
        const int r = c3_predict_wait(m, (int)(n_done % kRing));
        if (rc == 0) rc = r;
    }
    m->rows_call = false;
    if (m->tap_call) m->tap_call = false, m->tap_n = rc == 0 ? batch : 0;
    if (!first_error.empty()) g_err = first_error;
    return rc;
}

int c3_predict(c3_model *m, const void *x_host, int x_dtype, int64_t batch, float *y_host) {
    return predict_blocking(m, x_host, x_dtype, batch, nullptr, y_host);
}

// ---- one batch staged from several host buffers (the server of clair3_amd/serve.py: requests of several clients in one forward pass) ----
int c3_predict_submit_parts(c3_model *m, const void *const *parts, const int64_t *counts, int n_parts, int x_dtype, float *const *y_parts, int slot) {
    TRY(ring_ready(m, slot));
    if (n_parts < 1 || n_parts > kMaxParts) return fail("n_parts must be in [1, %d], got %d", kMaxParts, n_parts);
    if (!parts || !counts || !y_parts) return fail("null table: parts / counts / y_parts");
    if (x_dtype != C3_DTYPE_I8 && !(x_dtype == C3_DTYPE_I32 && m->kind == C3_KIND_PILEUP))
        return fail("windows must be int8%s (got dtype %d)", m->kind == C3_KIND_PILEUP ? " or int32" : "", x_dtype);
    RingInput in = ring_input(InKind::Parts, nullptr, x_dtype, 0, nullptr);
    for (int i = 0; i < n_parts; ++i) {
        if (counts[i] < 0) return fail("part %d: negative count %lld", i, (long long)counts[i]);
        if (counts[i] > 0 && (!parts[i] || !y_parts[i])) return fail("part %d: null buffer", i);
        in.batch += counts[i];
    }
    in.parts = parts, in.counts = counts, in.y_parts = y_parts, in.n_parts = n_parts;
    return predict_submit(m, in, slot);
}
int c3_predict_parts(c3_model *m, const void *const *parts, const int64_t *counts, int n_parts, int x_dtype, float *const *y_parts) {
    TRY(c3_predict_submit_parts(m, parts, counts, n_parts, x_dtype, y_parts, 0));
    return c3_predict_wait(m, 0);
}

// ---- depths: the reference's CPU-branch meaning of a pileup window (c3_rescale.h) ----
// what the *_depth entries refuse before anything is staged
static int depth_args_ok(c3_model *m, int x_dtype, int64_t batch, const int32_t *depth_host, bool region) {
    if (!m) return fail("null model");
    if (m->kind != C3_KIND_PILEUP) return fail("depths belong to pileup windows: a full-alignment model has no rescaling rule");
    if (batch < 0) return fail("negative batch");
    if (x_dtype == C3_DTYPE_I8)
        return fail("depths are refused for int8 counts: int8 tensor files are the reference's GPU branch, which does not rescale, and counts "
                    "above 127 have already wrapped in them -- pass int32%s counts", region ? " / int64" : "");
    if (x_dtype != C3_DTYPE_I32 && !(region && x_dtype == C3_DTYPE_I64))
        return fail("windows with depths must be int32%s (got dtype %d)", region ? " or int64 / size_t" : "", x_dtype);
    if (!depth_host && batch > 0) return fail("null depths (the entries without depths are c3_predict / c3_predict_submit / c3_predict_pileup_region)");
    return 0;
}

int c3_model_set_max_depth(c3_model *m, int max_depth) {
    if (!m) return fail("null model");
    if (m->kind != C3_KIND_PILEUP) return fail("max_depth belongs to the pileup network");
    if (max_depth <= 0) return fail("max_depth must be positive (got %d)", max_depth);
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("a prediction is in flight: call c3_predict_wait first");
    m->max_depth = max_depth;
    return 0;
}

int c3_predict_depth(c3_model *m, const void *x_host, int x_dtype, int64_t batch, const int32_t *depth_host, float *y_host) {
    TRY(depth_args_ok(m, x_dtype, batch, depth_host, false));
    return predict_blocking(m, x_host, x_dtype, batch, depth_host, y_host);
}

int c3_predict_submit_depth(c3_model *m, const void *x_host, int x_dtype, int64_t batch, const int32_t *depth_host, float *y_host, int slot) {
    TRY(depth_args_ok(m, x_dtype, batch, depth_host, false));
    return predict_submit(m, ring_input(InKind::Sliced, x_host, x_dtype, batch, y_host, depth_host), slot);
}

// ---- the region form of the pileup call on the ring ----
static int region_submit(c3_model *m, const char *who, const void *region_host, int x_dtype, int64_t n_cols, const int32_t *starts_host,
                         int64_t batch, const int32_t *depth_host, float *y_host, int slot) {
    if (!m) return fail("null model");
    if (m->kind != C3_KIND_PILEUP) return fail("%s needs a pileup model", who);
    if (batch < 0 || n_cols < 0) return fail("negative size");
    if (batch > 0 && (!region_host || !starts_host || !y_host)) return fail("null buffer");
    if (x_dtype != C3_DTYPE_I8 && x_dtype != C3_DTYPE_I32 && x_dtype != C3_DTYPE_I64)
        return fail("pileup regions must be int8, int32 or int64 / size_t (got dtype %d)", x_dtype);
    for (int64_t i = 0; i < batch; ++i)
        if (starts_host[i] < 0 || (int64_t)starts_host[i] + m->positions > n_cols)
            return fail("window %lld starts at column %d: outside the %lld-column region", (long long)i, starts_host[i], (long long)n_cols);
    RingInput in = ring_input(InKind::Region, region_host, x_dtype == C3_DTYPE_I64 ? C3_DTYPE_I32 : x_dtype, batch, y_host, depth_host);
    in.n_cols = n_cols, in.starts = starts_host, in.narrow = x_dtype == C3_DTYPE_I64;
    return predict_submit(m, in, slot);
}

int c3_predict_submit_region(c3_model *m, const void *region_host, int x_dtype, int64_t n_cols, const int32_t *starts_host, int64_t batch,
                             const int32_t *depth_host, float *y_host, int slot) {
    if (depth_host) TRY(depth_args_ok(m, x_dtype, batch, depth_host, true));
    return region_submit(m, "c3_predict_submit_region", region_host, x_dtype, n_cols, starts_host, batch, depth_host, y_host, slot);
}

// the two blocking region entries: submit + wait on slot 0 (so they pass through the range guard of c3_predict_wait like every other batch)
int c3_predict_pileup_region(c3_model *m, const void *region_host, int x_dtype, int64_t n_cols, const int32_t *starts_host,
                             int64_t batch, float *y_host) {
    if (m && m->kind == C3_KIND_PILEUP && batch == 0 && n_cols >= 0) return 0;
    TRY(region_submit(m, "c3_predict_pileup_region", region_host, x_dtype, n_cols, starts_host, batch, nullptr, y_host, 0));
    return c3_predict_wait(m, 0);
}

int c3_predict_pileup_region_depth(c3_model *m, const void *region_host, int x_dtype, int64_t n_cols, const int32_t *starts_host,
                                   int64_t batch, const int32_t *depth_host, float *y_host) {
    TRY(depth_args_ok(m, x_dtype, batch, depth_host, true));
    if (batch == 0 && n_cols >= 0) return 0;
    TRY(region_submit(m, "c3_predict_pileup_region_depth", region_host, x_dtype, n_cols, starts_host, batch, depth_host, y_host, 0));
    return c3_predict_wait(m, 0);
}

// ---- full-alignment windows as their occupied rows (c3_expand.h) ----
int c3_predict_submit_rows(c3_model *m, const void *rows_host, const int32_t *row_first, const int32_t *row_count, int64_t batch, float *y_host,
                           int slot) {
    TRY(ring_ready(m, slot));
    if (m->kind != C3_KIND_FULL_ALIGNMENT)
        return fail("rows belong to full-alignment windows: a pileup model has no zero rows to restore (c3_predict_submit takes its windows)");
    if (batch < 0) return fail("negative batch");
    if (batch > 0 && (!rows_host || !row_count || !y_host)) return fail("null buffer: rows / row_count / y_host");
    RingInput in = ring_input(InKind::Rows, rows_host, C3_DTYPE_I8, batch, y_host);
    in.row_first = row_first, in.row_count = row_count;
    for (int64_t b = 0; b < batch; ++b) {
        const int32_t c = table_i32(row_count, b);
        if (c < 0) return fail("window %lld: negative row_count %d", (long long)b, c);
        const int32_t first = row_first ? table_i32(row_first, b) : (m->depth - c) / 2;
        if (first < 0) return fail("window %lld: negative row_first %d", (long long)b, first);
        if ((int64_t)first + c > m->depth)
            return fail("window %lld: rows [%d, %lld) reach beyond the depth of %d rows", (long long)b, first, (long long)first + c, m->depth);
        in.rows_total += c;
    }
    return predict_submit(m, in, slot);
}

int c3_predict_rows(c3_model *m, const void *rows_host, const int32_t *row_first, const int32_t *row_count, int64_t batch, float *y_host) {
    TRY(c3_predict_submit_rows(m, rows_host, row_first, row_count, batch, y_host, 0));
    return c3_predict_wait(m, 0);
}

// plain host code (no device): what a caller that holds dense windows does to hand them over as rows
int64_t c3_pack_rows(int depth, int positions, int channels, const void *x_host, int64_t batch, void *rows_out, int32_t *row_first_out,
                     int32_t *row_count_out) {
    if (depth < 1 || positions < 1 || channels < 1) return fail("bad geometry %dx%dx%d", depth, positions, channels), -1;
    if (batch < 0) return fail("negative batch"), -1;
    if (batch > 0 && (!x_host || !row_first_out || !row_count_out)) return fail("null buffer: windows / row_first_out / row_count_out"), -1;
    const size_t row_bytes = (size_t)positions * channels, wbytes = (size_t)depth * row_bytes;
    int64_t total = 0;
    for (int64_t b = 0; b < batch; ++b) {
        const uint8_t *w = (const uint8_t *)x_host + (size_t)b * wbytes;
        int32_t first, count;
        occupied_run(w, depth, row_bytes, &first, &count);
        row_first_out[b] = first, row_count_out[b] = count;
        if (rows_out) memcpy((char *)rows_out + (size_t)total * row_bytes, w + (size_t)first * row_bytes, (size_t)count * row_bytes);
        total += count;
    }
    return total;
}

// ---- candidate positions instead of window starts (c3_select.h) ----
int c3_predict_submit_candidates(c3_model *m, const void *region_host, int x_dtype, int64_t n_cols, const int64_t *major_host,
                                 const int64_t *pos_host, const int32_t *depth_host, int64_t n_cand, int head_tail, float *y_host,
                                 uint8_t *status_host, int64_t *n_rows_host, int slot) {
    TRY(ring_ready(m, slot));
    if (m->kind != C3_KIND_PILEUP) return fail("candidate selection needs a pileup model: a full-alignment handle has no region matrix");
    if (n_cand < 0 || n_cols < 0) return fail("negative size");
    if (x_dtype == C3_DTYPE_I8)
        return fail("candidate selection is refused for int8 counts: int8 tensor files are the reference's GPU branch, whose windows are already "
                    "sliced -- pass the int32 / int64 region matrix");
    if (x_dtype != C3_DTYPE_I32 && x_dtype != C3_DTYPE_I64) return fail("the region matrix must be int32 or int64 / size_t (got dtype %d)", x_dtype);
    if (!n_rows_host) return fail("null buffer: n_rows_host");
    if (n_cols > 0 && (!region_host || !major_host)) return fail("null buffer: region / major");
    if (n_cand > 0 && (!pos_host || !y_host || !status_host)) return fail("null buffer: positions / rows / status");
    if (n_cand > INT32_MAX) return fail("too many candidates for one call (%lld)", (long long)n_cand);
    // the chunk table: one pass over major (8 bytes a column); the image column of a chunk's first follows from the layout
    CandInput ci;
    ci.pos = pos_host, ci.head_tail = head_tail != 0, ci.status_host = status_host, ci.n_rows_host = n_rows_host;
    const int64_t pad = ci.head_tail ? m->positions - 1 : 0;
    for (int64_t c = 0; c < n_cols; ++c) {
        if (c > 0 && major_host[c] <= major_host[c - 1])
            return fail("major must be strictly increasing: column %lld holds %lld after %lld", (long long)c, (long long)major_host[c],
                        (long long)major_host[c - 1]);
        if (c == 0 || major_host[c] != major_host[c - 1] + 1) {
            const int64_t k = (int64_t)ci.chunks.size();
            ci.chunks.push_back(SelectChunk{major_host[c], major_host[c], c + (2 * k + 1) * pad});
            ci.src_col.push_back(c);
        } else ci.chunks.back().last = major_host[c];
    }
    const int64_t img_cols = n_cols + 2 * pad * (int64_t)ci.chunks.size();
    if (img_cols > INT32_MAX - m->positions) return fail("region too large: %lld columns on the device", (long long)img_cols);
    if (depth_host) TRY(depth_args_ok(m, x_dtype, n_cand, depth_host, true));
    RingInput in = ring_input(InKind::Candidates, region_host, C3_DTYPE_I32, n_cand, y_host, depth_host);
    in.n_cols = img_cols, in.narrow = x_dtype == C3_DTYPE_I64, in.cand = &ci;
    if (n_cand == 0 || img_cols < m->positions) {  // no candidate, or no window fits: nothing to launch, every status is "no window"
        verify_count(m, n_cand, false);  // (verify mode: numbered like every submit, skipped when selected)
        record_batch(m, m->slot[slot], in, StagedBatch(), -1, false);
        return 0;
    }
    return predict_submit(m, in, slot);
}

int c3_predict_pileup_candidates(c3_model *m, const void *region_host, int x_dtype, int64_t n_cols, const int64_t *major_host,
                                 const int64_t *pos_host, const int32_t *depth_host, int64_t n_cand, int head_tail, float *y_host,
                                 uint8_t *status_host, int64_t *n_rows_host) {
    TRY(c3_predict_submit_candidates(m, region_host, x_dtype, n_cols, major_host, pos_host, depth_host, n_cand, head_tail, y_host, status_host,
                                     n_rows_host, 0));
    return c3_predict_wait(m, 0);
}

// ---- verify mode (c3_verify.h): the setting and the totals ----
static void verify_layers_zero(c3_model *m) {
    for (c3_verify_layer &t : m->vlayer) t = c3_verify_layer{}, t.worst_batch = -1;
    m->vlayer_batches = 0;
}
static void verify_zero(c3_model *m) {
    m->vstats = c3_verify_stats{};
    m->vstats.worst_batch = -1;
    m->vextra = c3_verify_extra{};
    verify_layers_zero(m);
}
int c3_model_set_verify(c3_model *m, int every, float tol, float near_tie, int policy) {
    if (!m) return fail("null model");
    if (every < 0) return fail("every must be >= 0 (0 = off), got %d", every);
    if (!(tol > 0.f)) return fail("tol must be > 0, got %g", (double)tol);
    if (!(near_tie >= 0.f)) return fail("near_tie must be >= 0, got %g", (double)near_tie);
    if (policy != C3_VERIFY_REPORT && policy != C3_VERIFY_ESCALATE && policy != C3_VERIFY_REPLACE)
        return fail("policy must be C3_VERIFY_REPORT, C3_VERIFY_ESCALATE or C3_VERIFY_REPLACE, got %d", policy);
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("a prediction is in flight: call c3_predict_wait first");
    if (every > 0 && m->refine_on)
        return fail("c3_model_set_verify: refine mode is on for this handle (c3_model_set_refine) and the two own the same rows: switch it off first");
    if (every > 0 && !m->verify_seen) verify_zero(m);
    m->verify_every = every, m->verify_tol = tol, m->verify_near_tie = near_tie, m->verify_policy = policy;
    m->verify_seen |= every > 0;
    return 0;
}
int c3_model_verify_stats(c3_model *m, c3_verify_stats *out) {
    if (!m || !out) return fail("null argument");
    *out = m->vstats;
    if (!m->verify_seen) out->worst_batch = -1;
    out->every = m->verify_every, out->policy = m->verify_policy, out->tol = m->verify_tol, out->near_tie = m->verify_near_tie;
    return 0;
}
int c3_model_verify_reset(c3_model *m) {
    if (!m) return fail("null model");
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("a prediction is in flight: call c3_predict_wait first");
    verify_zero(m);
    return 0;
}

// layer records (c3_verify.h): the switch, and the layers' totals in network order
int c3_model_set_verify_layers(c3_model *m, int enable) {
    if (!m) return fail("null model");
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("a prediction is in flight: call c3_predict_wait first");
    if (enable && !m->verify_layers_seen) verify_layers_zero(m);
    m->verify_layers = enable != 0, m->verify_layers_seen |= enable != 0;
    return 0;
}
int c3_model_verify_layers(c3_model *m, c3_verify_layer *out, int max_entries) {
    if (!m || (!out && max_entries > 0)) {
        fail("null argument");
        return -1;
    }
    if (!m->verify_layers_seen) return 0;
    int ids[kLayerMaxLayers];
    const int nl = verify_layer_ids(m, ids);
    for (int k = 0; k < nl && k < max_entries; ++k) {
        out[k] = m->vlayer[k];
        snprintf(out[k].name, sizeof(out[k].name), "%s", kTapName[ids[k]]);
        out[k].status = out[k].batches > 0 ? C3_VERIFY_LAYER_COMPARED : m->vlayer_batches > 0 ? C3_VERIFY_LAYER_FUSED : C3_VERIFY_LAYER_NONE;
    }
    return nl;
}

// ---- refine mode (c3_refine.h): the setting and the totals; the selection alone is c3_refine_select, behind the decoder entries ----
int c3_model_set_refine(c3_model *m, int enable, float gap) {
    if (!m) return fail("null model");
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("a prediction is in flight: call c3_predict_wait first");
    if (!enable) {
        m->refine_on = false;
        return 0;
    }
    if (!(gap >= 0.f) || !std::isfinite(gap)) return fail("c3_model_set_refine: gap must be a finite number >= 0, got %g", (double)gap);
    if (m->verify_every > 0)
        return fail("c3_model_set_refine: verify mode is on for this handle (c3_model_set_verify) and the two own the same rows: switch it off first");
    if (!m->exact.loaded)
        return fail("c3_model_set_refine: the exact form was not enabled at the last load: c3_model_set_exact(m, 1), then c3_model_load");
    if (!m->refine_seen) refine_zero(m);
    m->refine_on = m->refine_seen = true, m->refine_gap = gap;
    return 0;
}
int c3_model_refine_stats(c3_model *m, c3_refine_stats *out) {
    if (!m || !out) return fail("null argument");
    if (!m->refine_seen) refine_zero(m);
    *out = m->rfstats;
    out->gap = m->refine_gap;
    return 0;
}
int c3_model_refine_reset(c3_model *m) {
    if (!m) return fail("null model");
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("a prediction is in flight: call c3_predict_wait first");
    refine_zero(m);
    return 0;
}

// the handle's scratch buffer of the two decoder entries below: grown, never shrunk
static int ensure_decode_buf(c3_model *m, size_t bytes) {
    if (m->decode_bytes >= bytes) return 0;
    if (m->decode_dev) (void)hipFree(m->decode_dev);
    m->decode_dev = nullptr, m->decode_bytes = 0;
    HIP_TRY(hipMalloc(&m->decode_dev, bytes));
    m->decode_bytes = bytes;
    return 0;
}

int c3_outcome_maxima(c3_model *m, const float *y_host, int64_t batch, const uint8_t *ref21_host, float *maxp_host,
                      int32_t *argmax_host, uint8_t *early_host) {
    if (!m) return fail("null model");
    if (batch < 0) return fail("negative batch");
    if (batch == 0) return 0;
    if (!y_host || !ref21_host || !maxp_host || !argmax_host || !early_host) return fail("null buffer");
    for (int64_t i = 0; i < batch; ++i)
        if (ref21_host[i] != 0 && ref21_host[i] != 4 && ref21_host[i] != 7 && ref21_host[i] != 9)
            return fail("row %lld: reference gt21 index %d is not one of AA=0, CC=4, GG=7, TT=9", (long long)i, (int)ref21_host[i]);
    HIP_TRY(hipSetDevice(m->device));
    const size_t yb = (size_t)batch * m->nout * sizeof(float), rb = ((size_t)batch + 255) & ~(size_t)255;
    const size_t mb = (size_t)batch * kDecodeClasses * sizeof(float);
    const size_t total = yb + rb + 2 * mb + rb;
    TRY(ensure_decode_buf(m, total));
    char *base = (char *)m->decode_dev;
    float *y = (float *)base;
    uint8_t *ref = (uint8_t *)(base + yb);
    float *maxp = (float *)(base + yb + rb);
    int32_t *arg = (int32_t *)(base + yb + rb + mb);
    uint8_t *early = (uint8_t *)(base + yb + rb + 2 * mb);
    TRY(h2d_staged(y, y_host, yb, lane(m).stream));  // (pageable rows: through the bounce buffer, c3_model.h)
    TRY(h2d_staged(ref, ref21_host, (size_t)batch, lane(m).stream));
    DecodeParams dp{y, m->nout, ref, maxp, arg, early, nullptr, (int)batch, m->nout == 90 ? 1 : 0};
    hipLaunchKernelGGL(outcome_maxima_kernel<false>, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, lane(m).stream, dp);
    HIP_TRY(hipGetLastError());
    TRY(d2h_staged(maxp_host, maxp, mb, lane(m).stream));
    TRY(d2h_staged(argmax_host, arg, mb, lane(m).stream));
    TRY(d2h_staged(early_host, early, (size_t)batch, lane(m).stream));
    return 0;
}

int c3_decode_columns(c3_model *m, const float *y_host, int64_t batch, float *rows_host) {
    if (!m) return fail("null model");
    if (batch < 0) return fail("negative batch");
    if (batch == 0) return 0;
    if (!y_host || !rows_host) return fail("null buffer");
    HIP_TRY(hipSetDevice(m->device));
    const int wide = m->nout + kDecodeCols;
    const size_t total = (size_t)batch * wide * sizeof(float);
    TRY(ensure_decode_buf(m, total));
    float *rows = (float *)m->decode_dev;
    {   // the rows widen on their way through the bounce buffer (the kernel fills the decoder columns behind each)
        BounceBuf &b = bounce_buf();
        std::lock_guard<std::mutex> lk(b.mu);
        TRY(bounce_ready(b));
        const int64_t per = (int64_t)(BounceBuf::kBytes / ((size_t)wide * sizeof(float)));
        for (int64_t r0 = 0; r0 < batch; r0 += per) {
            const int64_t nr = std::min(per, batch - r0);
            for (int64_t r = 0; r < nr; ++r)
                memcpy((float *)b.pin + r * wide, y_host + (r0 + r) * m->nout, (size_t)m->nout * sizeof(float));
            HIP_TRY(hipMemcpyAsync(rows + r0 * wide, b.pin, (size_t)nr * wide * sizeof(float), hipMemcpyHostToDevice, lane(m).stream));
            HIP_TRY(hipStreamSynchronize(lane(m).stream));
        }
    }
    DecodeParams dp{rows, wide, nullptr, nullptr, nullptr, nullptr, rows + m->nout, (int)batch, m->nout == 90 ? 1 : 0};
    hipLaunchKernelGGL(outcome_maxima_kernel<true>, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, lane(m).stream, dp);
    HIP_TRY(hipGetLastError());
    TRY(d2h_staged(rows_host, rows, total, lane(m).stream));
    return 0;
}

// refine mode's selection on rows the caller brings (hand-made corners, another form's rows) without a forward pass: rows, scratch, record
// and list in the handle's decoder scratch, the two launches in the first lane
int c3_refine_select(c3_model *m, const float *rows_host, int row_floats, int64_t batch, float gap, int32_t *index_out, int64_t *n_out, float *gaps_out) {
    if (!m) return fail("null model");
    if (!n_out) return fail("null argument: n_out");
    if (batch < 0) return fail("negative batch");
    if (batch > kRefineMaxBatch) return fail("c3_refine_select: too many windows for one call (%lld)", (long long)batch);
    if (row_floats != m->nout && row_floats != m->nout + kDecodeCols)
        return fail("c3_refine_select: rows of %d floats: this model has %d probabilities, %d with the decoder columns", row_floats, m->nout, m->nout + kDecodeCols);
    if (!(gap >= 0.f) || !std::isfinite(gap)) return fail("c3_refine_select: gap must be a finite number >= 0, got %g", (double)gap);
    *n_out = 0;
    if (batch == 0) return 0;
    if (!rows_host || !index_out) return fail("null buffer: rows / index_out");
    HIP_TRY(hipSetDevice(m->device));
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const RefineScratch at(batch);
    const size_t yb = (size_t)batch * row_floats * sizeof(float), s_at = al(yb), r_at = al(s_at + at.bytes);
    TRY(ensure_decode_buf(m, r_at + kRefineRecordBytes + (size_t)batch * sizeof(int32_t)));
    TRY(use_lane(m, 0));
    hipStream_t s = lane(m).stream;
    char *base = (char *)m->decode_dev;
    TRY(h2d_staged(base, rows_host, yb, s));
    TRY(refine_select_launch(s, (const float *)base, row_floats, m->nout, batch, gap, base + s_at, base + r_at));
    RefineRecord rec;
    TRY(d2h_staged(&rec, base + r_at, sizeof(rec), s));
    if (rec.windows != (uint32_t)batch || rec.selected > rec.windows) return fail("internal: the refine record counts %u of %u windows selected", rec.selected, rec.windows);
    if (rec.selected) TRY(d2h_staged(index_out, base + r_at + kRefineRecordBytes, (size_t)rec.selected * sizeof(int32_t), s));
    if (gaps_out) TRY(d2h_staged(gaps_out, base + s_at, (size_t)batch * sizeof(float), s));
    *n_out = rec.selected;
    return 0;
}

// ---- score mode (c3_score.h): the setting and the entries ----
int c3_model_set_score(c3_model *m, int enable, float gamma, const float *class_weights) {
    if (!m) return fail("null model");
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("a prediction is in flight: call c3_predict_wait first");
    if (!enable) {
        m->score_on = m->score_census_on = false;  // (the census needs score mode; its totals stay readable)
        return 0;
    }
    if (!(gamma >= 0.f) || !std::isfinite(gamma)) return fail("gamma must be a finite number >= 0, got %g", (double)gamma);
    for (int c = 0; class_weights && c < m->nout; ++c)
        if (!std::isfinite(class_weights[c])) return fail("class weight %d is not finite (%g)", c, (double)class_weights[c]);
    m->score_on = true, m->score_gamma = (double)gamma, m->score_weighted = class_weights != nullptr;
    for (int c = 0; c < kScoreMaxCols; ++c) m->score_w[c] = class_weights && c < m->nout ? class_weights[c] : 1.f;
    return 0;
}
// ---- ... and its census (c3_census.h) ----
int c3_model_set_score_census(c3_model *m, int enable) {
    if (!m) return fail("null model");
    if (!m->score_on) return fail("c3_model_set_score_census: score mode is off for this handle: call c3_model_set_score first");
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("a prediction is in flight: call c3_predict_wait first");
    m->score_census_on = enable != 0;
    if (enable && !m->score_census_seen) m->score_census_seen = true, m->score_census = c3_score_census{}, m->score_census.tasks = m->nb;
    return 0;
}
static int census_entry_ok(const c3_model *m, const char *who) {
    if (!m) return fail("null model");
    if (!m->score_on) return fail("%s: score mode is off for this handle: call c3_model_set_score first", who);
    if (!m->score_census_seen) return fail("%s: the census was never enabled on this handle: call c3_model_set_score_census first", who);
    return 0;
}
int c3_score_census_read(c3_model *m, c3_score_census *out) {
    TRY(census_entry_ok(m, "c3_score_census_read"));
    if (!out) return fail("null argument: out");
    *out = m->score_census;
    return 0;
}
int c3_score_census_reset(c3_model *m) {
    TRY(census_entry_ok(m, "c3_score_census_reset"));
    m->score_census = c3_score_census{}, m->score_census.tasks = m->nb;
    return 0;
}
// what every score entry refuses first
static int score_args_ok(const c3_model *m, int label_dtype, int64_t batch, const char *who) {
    if (!m) return fail("null model");
    if (!m->score_on) return fail("%s: score mode is off for this handle: call c3_model_set_score first", who);
    if (label_dtype != C3_DTYPE_I8 && label_dtype != C3_DTYPE_F32) return fail("%s: labels must be int8 or float32 (got dtype %d)", who, label_dtype);
    if (batch < 0) return fail("negative batch");
    if (batch > ((int64_t)1 << 30)) return fail("%s: too many windows for one call (%lld)", who, (long long)batch);
    return 0;
}
static void score_result(const c3_model *m, const ScoreRecord &r, c3_score_result *out) {
    *out = c3_score_result{};
    out->windows = r.windows, out->tasks = m->nb, out->nonfinite = r.nonfinite;
    for (int k = 0; k < 4; ++k) out->loss_sum[k] = r.loss_sum[k], out->correct[k] = r.correct[k];
}
int c3_score_submit(c3_model *m, const void *x_host, int x_dtype, int64_t batch, const void *labels_host, int label_dtype, float *y_host,
                    float *loss_host, int slot) {
    TRY(score_args_ok(m, label_dtype, batch, "c3_score_submit"));
    if (batch > 0 && !labels_host) return fail("null buffer: labels");
    RingInput in = ring_input(InKind::Sliced, x_host, x_dtype, batch, y_host);
    in.score = true, in.labels = labels_host, in.label_dtype = label_dtype, in.loss_host = loss_host;
    return predict_submit(m, in, slot);
}
int c3_score_wait(c3_model *m, int slot, c3_score_result *out) {
    TRY(ring_ready(m, slot, false));
    if (!out) return fail("null argument: out");
    HostSlot &sl = m->slot[slot];
    if (!sl.busy) return fail("slot %d has nothing in flight", slot);
    if (!sl.scored) return fail("slot %d holds a batch that is not scored: c3_predict_wait completes it", slot);
    TRY(c3_predict_wait(m, slot));
    score_result(m, sl.score_rec, out);
    return 0;
}
// blocking: a batch of two chunks or more (predict_chunk) travels as chunks through three slots of the ring; the chunks' records are added up
// here in chunk order (the sums of a batch therefore depend on the cut at the level of double rounding, the windows' values do not)
int c3_score(c3_model *m, const void *x_host, int x_dtype, int64_t batch, const void *labels_host, int label_dtype, float *y_host, float *loss_host,
             c3_score_result *out) {
    TRY(score_args_ok(m, label_dtype, batch, "c3_score"));
    if (!out) return fail("null argument: out");
    const int64_t chunk = predict_chunk(m);
    if (chunk <= 0 || batch < 2 * chunk) {
        TRY(c3_score_submit(m, x_host, x_dtype, batch, labels_host, label_dtype, y_host, loss_host, 0));
        return c3_score_wait(m, 0, out);
    }
    constexpr int kRing = 3;
    const int64_t wbytes = c3_model_window_bytes(m, x_dtype), lbytes = (int64_t)m->nout * (label_dtype == C3_DTYPE_F32 ? 4 : 1);
    c3_score_result total = c3_score_result{}, one;
    total.tasks = m->nb;
    auto add = [&](const c3_score_result &r) {
        total.windows += r.windows, total.nonfinite += r.nonfinite;
        for (int k = 0; k < 4; ++k) total.loss_sum[k] += r.loss_sum[k], total.correct[k] += r.correct[k];
    };
    int64_t n_sub = 0, n_done = 0;
    int rc = 0;
    for (int64_t off = 0; off < batch && rc == 0; ++n_sub) {
        const int64_t take = batch - off < 2 * chunk ? batch - off : chunk;  // (a tail shorter than a chunk joins the last one)
        if (n_sub - n_done == kRing && (rc = c3_score_wait(m, (int)(n_done++ % kRing), &one)) == 0) add(one);
        if (rc == 0)
            rc = c3_score_submit(m, (const char *)x_host + off * wbytes, x_dtype, take, (const char *)labels_host + off * lbytes, label_dtype,
                                 y_host ? y_host + off * m->row : nullptr, loss_host ? loss_host + off * m->nb : nullptr, (int)(n_sub % kRing));
        if (rc != 0) break;
        off += take;
    }
    const std::string first_error = rc != 0 ? g_err : std::string();
    for (; n_done < n_sub; ++n_done) {  // drain, also after an error: no slot stays busy behind a failed call
        const int r = c3_score_wait(m, (int)(n_done % kRing), &one);
        if (r == 0 && rc == 0) add(one);
        if (rc == 0) rc = r;
    }
    if (!first_error.empty()) g_err = first_error;
    if (rc == 0) *out = total;
    return rc;
}
// given probability rows (the reference's, the exact form's rounded, adversarial ones) without a forward pass: rows, labels, partials,
// record and values in the handle's decoder scratch, the two launches in the first lane
int c3_score_rows(c3_model *m, const float *rows_host, int row_floats, int64_t batch, const void *labels_host, int label_dtype, c3_score_result *out,
                  float *loss_host) {
    TRY(score_args_ok(m, label_dtype, batch, "c3_score_rows"));
    if (!out) return fail("null argument: out");
    if (row_floats < m->nout) return fail("c3_score_rows: rows of %d floats are shorter than the %d probabilities of this model", row_floats, m->nout);
    ScoreRecord rec = ScoreRecord{};
    if (batch == 0) return score_result(m, rec, out), 0;
    if (!rows_host || !labels_host) return fail("null buffer: rows / labels");
    HIP_TRY(hipSetDevice(m->device));
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t yb = (size_t)batch * row_floats * sizeof(float), lb = (size_t)batch * m->nout * (label_dtype == C3_DTYPE_F32 ? 4 : 1);
    const size_t vb = (size_t)batch * m->nb * sizeof(float);
    const size_t l_at = al(yb), p_at = al(l_at + lb), r_at = p_at + kScorePartBytes, v_at = r_at + kScoreRecordBytes;
    const size_t c_at = al(v_at + vb), cb = m->score_census_on ? sizeof(ScoreCensusTable) : 0;  // (the census: its table behind the values)
    TRY(ensure_decode_buf(m, cb ? c_at + cb : v_at + vb));
    TRY(use_lane(m, 0));
    hipStream_t s = lane(m).stream;
    char *base = (char *)m->decode_dev;
    TRY(h2d_staged(base, rows_host, yb, s));
    TRY(h2d_staged(base + l_at, labels_host, lb, s));
    TRY(score_launch(m, s, (const float *)base, row_floats, base + l_at, label_dtype, batch, (float *)(base + v_at), (uint64_t *)(base + p_at),
                     (ScoreRecord *)(base + r_at)));
    if (cb) TRY(census_launch(m, s, (const float *)base, row_floats, base + l_at, label_dtype, batch, (ScoreCensusTable *)(base + c_at)));
    TRY(d2h_staged(&rec, base + r_at, sizeof(rec), s));
    if (loss_host) TRY(d2h_staged(loss_host, base + v_at, vb, s));
    if (cb) {
        ScoreCensusTable t;
        TRY(d2h_staged(&t, base + c_at, sizeof(t), s));
        census_add(m->score_census, t, batch, m->nb);
    }
    score_result(m, rec, out);
    return 0;
}

}  // extern "C"
