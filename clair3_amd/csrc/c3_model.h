// c3_model.h -- the model handle of libc3hip.so and the helpers every host-side unit shares: error convention, device
// memory, the profiling scope, the launch wrapper of the tiled contraction.
//
// The host side of the library is one translation unit (c3_model.hip) made of:
//   c3_model.h     this file
//   c3_pack.h      c3_model_load: BatchNorm folding, gate re-ordering, matrix-instruction fragment layouts, fp16 pieces
//   c3_forward.h   the launch sequences of the two forward passes (clair3/model.py:130-161 and :377-416)
//   c3_mixed.h     the boundary forms of a per-layer precision plan: fp32 forms that read / write plane activations between product layers
//   c3_hostring.h  the host <-> device ring behind c3_predict / c3_predict_submit / _wait.  predict_submit is one sequence for every input
//                  kind (sliced windows, a region with starts, candidates, occupied rows handed over or packed here): lane and shared-chip
//                  forms, plan_batch (THE layout of a staged batch: StagedBatch below), ensure_slot, fill_<kind>, queue_input, launch_batch,
//                  record_batch; c3_predict_wait and the range guard's one re-run (range_guard_rerun) read the slot's plan.  Behind them the
//                  entries: per-window depths (c3_rescale.h), regions, candidates (c3_select.h), rows (c3_expand.h), the two decoder entries
//   c3_comm.h      the gather of a sharded job on RCCL
//   c3_verify.h    verify mode's two compare kernels and their record (included with the other kernels below): a selected batch of the ring
//                  runs a second forward pass on the fp32 forms from the same staged input (c3_hostring.h shadow_pass) and the two sets of
//                  rows are compared on the device; with c3_model_set_verify_layers also the two forms' outputs of every layer (layer_compare_kernel)
//   c3_score.h     score mode's two kernels and their record: the focal loss and arg-max accuracy of a labelled batch on the rows that answer
//                  it (c3_hostring.h run_score; the entries c3_score_submit / _wait, c3_score, c3_score_rows sit at the end of that file)
//   c3_census.h    score mode's census: the kernel that counts a scored batch's confusion, reliability and gap tables from the same rows, and
//                  the batch's table (c3_hostring.h run_census; the entries c3_model_set_score_census, c3_score_census_read / _reset)
//   c3_refine.h    refine mode: the kernels that find the windows of a batch near a tie, gather them for the exact form and put the refined
//                  rows back (c3_hostring.h run_refine_select, c3_predict_wait; c3_exact.h refine_pass; the entries c3_model_set_refine, ...)
//   c3_debug.h     c3_debug_* / c3_profile_* (parity tests, bench.py)
//   c3_calibrate.h full alignment: channel exponents calibrated from observed activations -- the census kernel and pass, the rule, the entries;
//                  the packing part of a full-alignment load (fa_pack_weights) and, on it, the range guard's policy C3_RANGE_RECALIBRATE: a trip
//                  takes the census during its fp32 re-run, solves, packs again and stays on the product forms (range_guard_recalibrate)
//   c3_exact.h     the exact form: both networks in fp64 on the device, its kernels, workspace and entries (c3_predict_exact, c3_exact_fetch);
//                  on the ring: exact_ring_pass (c3_model_set_answer), exact_shadow_pass (c3_model_set_verify_reference), verify_replace_launch
//   c3_model.hip   create / geometry / device-resident entries / describe / destroy
// Every layer has exactly two forms: the product (fp16x3 split products on the 16-bit matrix instructions) and
// one fp32-MFMA form that the range guard falls back to (and that C3HIP_FP32=1 selects from the start).
#pragma once
#include <hip/hip_runtime.h>
#include <errno.h>
#include <sys/mman.h>

#include <algorithm>
#include <functional>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/c3hip.h"
#include "c3_gemm.h"
#include "c3_kernels.h"
#include "c3_conv1.h"
#include "c3_tail.h"
#include "c3_decode.h"
#include "c3_lstm_fused.h"
#include "c3_rescale.h"
#include "c3_select.h"
#include "c3_expand.h"
#include "c3_host.h"
#include "c3_conv3.h"
#include "c3_conv3s2.h"
#include "c3_conv3w.h"
#include "c3_l4.h"
#include "c3_dense.h"
#include "c3_verify.h"
#include "c3_score.h"
#include "c3_census.h"
#include "c3_refine.h"

using namespace c3;

// ------------------------------------------------------------------------------------------ errors
static thread_local std::string g_err;
static int fail(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}
#define HIP_TRY(expr)                                                                                    \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define TRY(expr)            \
    do {                     \
        int rc_ = (expr);    \
        if (rc_) return rc_; \
    } while (0)

// ------------------------------------------------------------------------------------------ model
static const int kHeadN[4] = {21, 3, 33, 33};
static const char *kHeadName[4] = {"Y_gt21_logits", "Y_genotype_logits", "Y_indel_length_logits_1",
                                   "Y_indel_length_logits_2"};
static const char *kConvName[9] = {"conv1.conv",         "res_block1.0.conv1", "res_block1.0.conv2",
                                   "conv3.conv",         "res_block2.0.conv1", "res_block2.0.conv2",
                                   "conv5.conv",         "res_block3.0.conv1", "res_block3.0.conv2"};
static const char *kBnName[9] = {"conv1.bn",         "res_block1.0.bn1", "res_block1.0.bn2",
                                 "conv3.bn",         "res_block2.0.bn1", "res_block2.0.bn2",
                                 "conv5.bn",         "res_block3.0.bn1", "res_block3.0.bn2"};
static const int kConvCout[9] = {64, 64, 64, 128, 128, 128, 256, 256, 256};
static const int kConvStride[9] = {2, 1, 1, 2, 1, 1, 2, 1, 1};
static const char *kFaLayerTag[9] = {"fa.conv1", "fa.res1a", "fa.res1b", "fa.conv3", "fa.res2a",
                                     "fa.res2b", "fa.conv5", "fa.res3a", "fa.res3b"};
// tensors c3_debug_tap can capture: full alignment act0 .. act8 (= their index), spp, l4_out; pileup l4_out, lstm1_out, gx2, lstm2_out
enum { kTapSpp = 9, kTapL4 = 10, kTapLstm1 = 11, kTapGx2 = 12, kTapLstm2 = 13, kTapCount = 14 };
static const char *kTapName[kTapCount] = {"act0", "act1", "act2", "act3", "act4", "act5", "act6", "act7", "act8",
                                          "spp",  "l4_out", "lstm1_out", "gx2", "lstm2_out"};

// ---- the per-layer precision plan (c3_model_set_layer_precision): one bit per named layer; a layer takes its product form iff
// layer_f16(m, bit).  Full alignment: bit l = convolution l, kLayerL4 behind them; pileup: its three layers behind that
enum { kLayerL4 = 1u << 9, kLayerLstm1 = 1u << 10, kLayerProj2 = 1u << 11, kLayerLstm2 = 1u << 12 };
struct LayerName { const char *name; uint32_t bit; };
// the names of a kind in network order (the kFaLayerTag / ProfScope tags without their prefix); the FC tail is fp32 in both forms and has none
static const LayerName kPileupLayers[] = {{"lstm1", kLayerLstm1}, {"proj2", kLayerProj2}, {"lstm2", kLayerLstm2}, {"l4", kLayerL4}};
static const LayerName kFaLayers[] = {{"conv1", 1u << 0}, {"res1a", 1u << 1}, {"res1b", 1u << 2}, {"conv3", 1u << 3}, {"res2a", 1u << 4}, {"res2b", 1u << 5},
                                      {"conv5", 1u << 6}, {"res3a", 1u << 7}, {"res3b", 1u << 8}, {"l4", kLayerL4}};
static int layer_names(int kind, const LayerName **out) {
    if (kind == C3_KIND_PILEUP) return *out = kPileupLayers, (int)(sizeof(kPileupLayers) / sizeof(LayerName));
    if (kind == C3_KIND_FULL_ALIGNMENT) return *out = kFaLayers, (int)(sizeof(kFaLayers) / sizeof(LayerName));
    return *out = nullptr, 0;
}
static uint32_t layer_mask_all(int kind) {
    const LayerName *t;
    uint32_t all = 0;
    for (int i = 0, n = layer_names(kind, &t); i < n; ++i) all |= t[i].bit;
    return all;
}
// "conv3,res2a" of a mask, network order ("" = none)
static std::string layer_mask_text(int kind, uint32_t mask) {
    const LayerName *t;
    std::string out;
    for (int i = 0, n = layer_names(kind, &t); i < n; ++i)
        if (mask & t[i].bit) out += (out.empty() ? "" : ","), out += t[i].name;
    return out;
}

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

struct ProfRec {
    std::string name;
    hipEvent_t a, b;
    double flops, bytes;
    double mfma_flops = 0.0;  // FLOP the matrix instructions of the launch EXECUTE (tile padding, piece products included)
    double mfma_peak = 0.0;   // dense peak (TFLOP/s) of the matrix instruction the launch issues: 2500 (16-bit) or 157.3 (fp32)
};

// ---- one batch of the submit / wait ring as it is staged (c3_hostring.h plan_batch works every field out before anything is copied) ----
struct Section { size_t off = 0, bytes = 0; };  // (a section the batch's kind does not use: bytes == 0)
struct StagedBatch {
    // the slot's input buffer (pin_x -> dev_x), in this order, every section from a multiple of 256 bytes
    Section image;      // sliced windows | the region matrix (a candidate batch: the device image) | the occupied rows of full-alignment windows
    Section cand_pos;   // candidates: their int64 positions
    Section depth_in;   // candidates: their depths as handed over (the selection compacts them into `depth`)
    Section chunks;     // candidates: the chunk table (SelectChunk) -- the last section a candidate batch stages
    Section starts;     // window starts of a region batch (staged) / of the kept candidates (written by the selection kernels)
    Section depth;      // per-window depths as the kernels read them: staged, or compacted by the selection (only when a window is deep)
    Section start_all;  // candidates: every candidate's start
    Section tiles;      // candidates: the compaction tiles' counts
    Section rows_tab;   // a rows batch: one ExpandEntry per window.  A batch packed here (C3HIP_PACK_ROWS=1) by ONE range moves it, `tail`
                        // and `staged` down behind the rows it found (fill_packed_rows) -- the only values settled after the plan
    Section labels;     // a scored batch (c3_score.h): its labels (batch, nout), int8 or float32 -- the last section a scored batch stages
    size_t tail = 0;    // [tail, staged): what is staged behind the image
    size_t staged = 0;  // bytes of the input buffer that cross PCIe
    size_t x_cap = 0;   // bytes the slot's input buffers must hold
    // the slot's output buffer (dev_y -> pin_y)
    Section y;          // the rows
    Section status;     // candidates: one status byte each
    Section kept;       // candidates: the count of kept candidates (16 bytes from a multiple of 16)
    Section verify;     // a verified batch (c3_verify.h): its VerifyRecord, behind the kept count (rows that stay on the device: the only section)
    Section layers;     // ... with layer records (c3_model_set_verify_layers): one LayerRecord per layer in network order, behind the verify record
    Section score;      // a scored batch (c3_score.h): its ScoreRecord, behind everything above
    Section losses;     // ... and the windows' values [batch][tasks] float32 behind the record, when the caller asked for them
    Section census;     // ... and the batch's ScoreCensusTable (c3_census.h) behind those, from a multiple of 256 bytes: only with the census on
    Section refine;     // refine mode (c3_refine.h): the batch's RefineRecord and int32[batch] selected windows behind everything above (rows that stay
                        // on the device: the only section) -- only while the mode is on, for a batch it covers
    size_t y_total = 0;
    bool gather_only = false;  // a region / candidate batch the exact form reads (c3_exact.h exact_ring_pass): `depth` is staged (zeros where the
                               // caller gave none) only so that the pre-pass of c3_rescale.h gathers its windows; the product forms do not see it
};

constexpr int kMaxParts = 64;  // host buffers one staged batch may be assembled from (C3_MAX_PARTS)

struct HostSlot {
    void *pin_x = nullptr;
    float *pin_y = nullptr;
    void *dev_x = nullptr;
    float *dev_y = nullptr;
    size_t cap_x = 0, cap_y = 0;
    hipEvent_t ev_h2d = nullptr, ev_out = nullptr;
    uint32_t *pin_flag = nullptr;  // pinned copy of the model's range_flag after this batch
    // ---- the batch in flight (c3_hostring.h record_batch) ----
    bool busy = false;
    // its layout.  Window starts, depths and the rows table stay on the device with the slot (behind the counts in dev_x): the range guard's
    // re-run gathers, rescales and expands again from the ORIGINAL counts (the pre-passes never write dev_x)
    StagedBatch plan;
    int64_t batch = 0;
    int x_dtype = 0, lane = 0;  // lane: the lane (Lane) the batch in flight runs in
    float *y_host = nullptr, *y_dev_out = nullptr;  // y_dev_out (c3_predict_submit_dev): the rows stay in the caller's device buffer
    int64_t tap_off = 0;  // first window of this batch in the c3_predict call it is a piece of (debug taps)
    bool used_f16 = false;  // the batch in flight was computed by the fp16x3 kernels (c3_predict_wait then checks its range)
    uint64_t pack_epoch = 0;  // ... with the weights of this packing (c3_model pack_epoch: the range guard's recalibration moves it on)
    int64_t rows_shipped = -1;  // rows staged for the batch in flight (-1: a dense batch)
    // a candidate batch (c3_select.h; c3_predict_submit_candidates): the statuses and the count of kept candidates leave behind the rows
    bool cand = false, cand_none = false;  // cand_none: nothing was launched: no candidate, or a region in which no window fits -- every status is "no window"
    uint8_t *status_host = nullptr;
    int64_t *n_rows_host = nullptr;
    int64_t n_chunks = 0;
    // a batch of parts (c3_predict_submit_parts): rows [sum(part_count[0 .. i)), + part_count[i]) of the batch belong at part_y[i].  The caller's
    // tables are copied here: they may be reused as soon as submit returns
    int n_parts = 0;  // 0: a batch from one buffer, its rows go to y_host
    int64_t part_count[kMaxParts] = {};
    float *part_y[kMaxParts] = {};
    // a verified batch (c3_verify.h): the rows of its second pass on the fp32 forms, the compare kernel's partials behind them.  The buffer
    // belongs to the SLOT, not to the lane: two slots in flight in one lane would overwrite each other's rows before c3_predict_wait reads them
    bool verified = false;
    int64_t verify_ordinal = 0;  // which submit of the handle this batch was (c3_verify_stats.worst_batch)
    float *shadow = nullptr;
    size_t shadow_bytes = 0, shadow_part = 0;  // shadow_part: offset of the partials
    // ... against the exact form (C3_VERIFY_REF_EXACT): the float32 rounding of the exact rows at the front of `shadow` (what an escalated or
    // repaired batch is answered with), the fp64 rows of the whole batch at shadow_rows64, the fp64 compare kernel's partials at shadow_part
    size_t shadow_rows64 = 0;
    // ... with layer records: the product pass's layer outputs of the whole batch (copied behind the producing launches like a tap's, never
    // into a user's tap buffers) and the layer compare kernel's partials.  The slot's like the shadow rows, allocated on first use
    float *layer_buf[kTapCount] = {};
    size_t layer_bytes[kTapCount] = {};
    LayerRecord *layer_part = nullptr;
    int layer_part_stride = 0;               // partials per layer the buffer holds
    uint32_t layer_kept = 0, layer_planes = 0;  // of the batch in flight: tensors the product pass produced / as planes
    bool layer_dropped = false;               // ... a buffer for them could not be allocated: the batch brings no layer record
    int layer_parts[kTapCount] = {};          // ... and the partials written per tensor so far
    // a scored batch (c3_score.h; c3_score_submit): the score kernel's partials are the slot's, allocated on first use.  rows_home: the caller
    // wants no rows (y_host == NULL) -- they stay in dev_y, are scanned there for the range guard, and only the record and the windows' values leave
    bool scored = false, rows_home = false;
    int label_dtype = 0;
    float *loss_host = nullptr;
    uint64_t *score_part = nullptr;
    ScoreRecord score_rec = {};  // of the batch c3_predict_wait completed last (c3_score_wait hands it over)
    // refine mode (c3_refine.h): refine_on -- the mode was on when the batch in flight was submitted (it counts in the totals, refined or
    // skipped); the selection's scratch (RefineScratch) is the slot's, allocated on first use
    bool refine_on = false;
    void *refine_scratch = nullptr;
    size_t refine_scratch_bytes = 0;
    // a section of the staged batch on the device / in the pinned input buffer (nullptr: the batch has none)
    template <class T> T *dev(const Section &s) const { return s.bytes ? (T *)((char *)dev_x + s.off) : nullptr; }
    template <class T> T *pin(const Section &s) const { return s.bytes ? (T *)((char *)pin_x + s.off) : nullptr; }
};

constexpr int kHostSlots = 4;  // batches in flight per handle through c3_predict_submit / _wait (C3_HOST_SLOTS)

// ---- the ring's lanes (round 6) ----
// Batches of the submit / wait ring used to run strictly one after the other: ONE workspace and ONE kernel stream per handle.  A lane is
// everything a forward pass writes -- the workspace and the kernel stream: with two or three of them consecutive small batches (dealt to the
// lanes in submit order, c3_hostring.h) overlap on the chip (what three HANDLES in flight do, 876 k against 735 k windows/s at B = 256,
// without a second copy of the weights) and fill each other's under-filled launches.  Rows do not depend on the lane
// (same kernels, same data).  env C3HIP_RING_LANES=1: one lane.
struct Lane {
    hipStream_t stream = nullptr;  // kernels (and the rows on their way out)
    int64_t cap = 0;               // windows per micro-batch the workspace can hold
    bool last_planes = false;      // the last forward pass left plane activations in act[] / h1 (c3_debug_fetch converts)
    std::vector<DevBuf> bufs;
    float *act[9] = {};
    float *spp = nullptr, *part = nullptr, *l4dbg = nullptr;
    float *h1 = nullptr, *gx2 = nullptr, *h2 = nullptr;
    int64_t last_n = 0;  // windows of the last micro-batch (for debug fetch)
    int32_t *xr = nullptr;  // rescaled sliced int32 windows of a micro-batch that carries depths (c3_rescale.h); allocated on first use
    int64_t xr_cap = 0;     // windows it holds
    int8_t *xe = nullptr;   // dense int8 windows of a micro-batch that came as occupied rows (c3_expand.h); allocated on first use
    int64_t xe_cap = 0;     // windows it holds
    void *xo = nullptr;     // dense pileup windows of a micro-batch that occlusion mode builds (c3_occlude.h); allocated on first use
    int64_t xo_cap = 0;     // int32 windows it holds
};
// ---- the exact form (c3_exact.h): never enabled = nothing allocated, uploaded or launched ----
struct ExactState {
    bool want = false;    // c3_model_set_exact: the next loads also place the double weights
    bool loaded = false;  // the last load did
    std::vector<void *> weights;  // every device allocation of the double weights (c3_pack.h pack_exact)
    double *wih[2] = {}, *pb[2] = {}, *whh[2] = {};  // pileup: W_ih [2 * 4H][in], b_ih + b_hh [2 * 4H] in PyTorch row order; W_hh as exact_lstm_kernel fragments
    double *cw[9] = {}, *cb[9] = {};                 // full alignment: [Cout][tap][Cin] and [Cout], BatchNorm folded in double
    double *l4w = nullptr, *l4b = nullptr, *w5 = nullptr, *b5 = nullptr, *wh = nullptr, *bh = nullptr;  // L4 [FC][K4]; L5_k stacked [nb * 128][FC]; heads stacked [nout][128]
    // the workspace of a pass (c3_exact.h states the sizes): the staged windows, every layer output, the rows
    std::vector<void *> ws;
    int64_t cap = 0;            // windows a pass can hold
    size_t x_window_bytes = 0;  // ... of up to this many bytes each
    void *x = nullptr;
    double *act[9] = {}, *spp = nullptr, *gx1 = nullptr, *h1 = nullptr, *gx2 = nullptr, *h2 = nullptr;
    double *l4 = nullptr, *l5 = nullptr, *logit = nullptr, *y = nullptr;
    int64_t last_n = 0;  // windows of the last pass of the last call (c3_exact_fetch)
    // on the ring (exact_ring_pass): ONE workspace for all lanes, so the passes of different lanes are put in order by this event, recorded
    // behind each pass and waited on by the next; created when the exact form is first used on the ring
    hipEvent_t ring_ev = nullptr;
    bool ring_recorded = false;
};
// a tensor of the last c3_model_load as the handle keeps it while the range-guard policy is RECALIBRATE
struct KeptTensor {
    std::string name;
    std::vector<int64_t> shape;
    std::vector<float> data;
};
constexpr int kCalChannels = 896;  // the channels of the six groups of c3_pack.h FaChannelExps: 2 x (64 + 128 + 256)
constexpr int kMaxLanes = 3;  // = the batches a worker keeps in flight (ring of three slots)

struct c3_model {
    int kind = 0, C = 0, add_indel = 0, device = 0;
    int depth = 89, positions = 33;
    int nb = 2, nout = 24;
    int row = 24;  // floats per output row: nout, + kDecodeCols when c3_model_set_decode_columns is on
    bool loaded = false;
    hipStream_t h2d_stream = nullptr;  // staged windows on their way in (the kernel streams are the lanes', below)

    // ---- packed weights (device) ----
    // pileup
    float *proj_w[2] = {nullptr, nullptr};  // LSTM input projections [2*4H][Kp] fp32 (layer 1: the fp32 form of the LSTM2 projection)
    float *proj_b[2] = {nullptr, nullptr};  // [2*4H], b_ih + b_hh
    float *whh[2] = {nullptr, nullptr};     // W_hh as fp32 matrix-instruction fragments (fp32 forms)
    float *whh16[2] = {nullptr, nullptr};   // W_hh as two fp16 pieces in the same fragment order (c3_kernels.h, c3_lstm_fused.h)
    float *l1_wih = nullptr, *l1_bias = nullptr;  // LSTM1 input projection as fragments of the fused kernel (fp32; int32 windows)
    float *l1_wih16 = nullptr;                    // the same as two fp16 pieces of 128 W_ih (int8 windows)
    float *proj2_pw = nullptr;   // LSTM2 projection weights as dense_planes_pipe_kernel chunks (c3_dense.h)
    float *proj2_pwr = nullptr;  // the same in the register-fragment order of dense_planes_wres_kernel
    float *proj2_post = nullptr; // [1280] x 2^-k, one power of two for the whole matrix (c3_pack.h), as the vector dense_planes_pipe_kernel reads
    float proj2_post_scale = 1.f;  // the same 2^-k for dense_planes_wres_kernel
    // full alignment
    float *conv_w[9] = {};   // [Cout][9 Cin] fp32, BatchNorm folded (conv1: [64][3][32], /100 folded): the fp32 forms
    float *conv_b[9] = {};
    float *conv1_w16 = nullptr;  // conv1 of a window with C != 8 as two fp16 pieces for the tiled contraction (keep mode of the 9-channel model)
    float *conv1_w16_post = nullptr;  // its [64] per-channel 2^-k
    float *conv1_wfrag16 = nullptr;  // conv1 as fragments of conv1_i8_f16_kernel / conv3x3_planes_kernel's SRC8 forms (C = 8 or 9)
    float *conv1_post = nullptr;     // their [64] per-channel 2^-k
    float *pconv_w[9] = {};  // stride-1 convs: conv3x3_planes_kernel chunks in fragment order [Cout/64][Cin/64][9][2][4][2][64 lanes x 16 B];
                             // stride-2 convs: conv3x3_s2_planes_kernel chunks, the same fragment order [Cout/64][9 Cin/64][2][4][2][64 lanes x 16 B]
    float *pconv_pre[9] = {}, *pconv_post[9] = {};  // [Cout] the output channels' powers of two 2^k / 2^-k (c3_pack.h row_scales)
    float *wconv_w[9] = {};     // stride-1 convs: the F(2,3)-along-H weights U of conv3x3_wino_planes_kernel (c3_conv3w.h) in fragment
                                // order [Cout/64][Cin/32][12 taps][2][2][2][64 lanes x 16 B]
    float *wconv_post[9] = {};  // [Cout] 2^-k of U's rows
    // shared FC tail
    float *l4_w = nullptr, *l4_b = nullptr;  // [FC][K4] native layout (fp32 form)
    float *l4_wf = nullptr;                  // the same as two fp16 pieces in fragment order (c3_l4.h), every feature row times its power of two
    float *l4_pre = nullptr, *l4_post = nullptr;  // [FC] 2^k / 2^-k
    float *b5 = nullptr;
    float *w5f = nullptr, *whf = nullptr, *bh48 = nullptr;  // L5 / head weights as fragments of fc_tail_mfma_kernel (c3_tail.h)
    std::vector<int> act_exp[9];  // channel equalisation (c3_pack.h): activation channel c of layer l lives on the device times 2^act_exp[l][c]
    float *zeros = nullptr;  // 256-byte zero page: padding taps of the conv loaders read from here
    int FC = 0, K4 = 0;

    // ---- arithmetic ----
    uint32_t *range_flag = nullptr;  // device word set by the fp16x3 kernels when an activation nears the fp16 range (c3_gemm.h kF16Range)
    uint32_t *pin_flag = nullptr;    // pinned copy of range_flag for c3_predict_device_checked
    bool f16_ok = true;              // cleared when a batch came back out of range / non-finite (or by C3HIP_FP32=1): every layer then runs its fp32-MFMA form
    // The per-layer plan: layers that run their fp32-MFMA form while the rest of the handle stays on fp16x3 (0 = none: nothing changes).
    // plan: what the caller named (c3_model_set_layer_precision, C3HIP_FP32_LAYERS; survives a load); auto: what the load-time rule below
    // escalated INSTEAD of the whole handle (C3HIP_AUTO_FP32_LAYERS; decided again by every load)
    uint32_t fp32_plan = 0, fp32_auto = 0;
    uint32_t auto_layers = 0;        // C3HIP_AUTO_FP32_LAYERS: the layers the load-time rule escalates (0 = unset: the whole handle)
    std::string precision_text;      // storage of precision = "fp32-auto(<layers>)"
    // Precision escalation decided at c3_model_load (pileup only, c3_pack.h lstm_sensitivity): a recurrence whose weights hold an entry of
    // magnitude >= auto_fp32_at amplifies the 2^-22 of the fp16 piece pairs over its 33 steps beyond north_star's 1e-4 on rare windows
    // (tests/diag/sensitive_window.py), so such a handle STARTS on the fp32 matrix instructions.  C3HIP_FP32 set (0 or 1) is an explicit
    // choice and switches the automatism off; C3HIP_AUTO_FP32=<threshold> moves it (0 = never).
    bool precision_forced = false;   // C3HIP_FP32 was given
    bool forced_f16 = true;          // ... and what it chose (0: fp16x3, 1: fp32): every c3_model_load starts from it again
    float auto_fp32_at = 4.0f;
    float lstm_wmax = 0.f;           // max |w| over W_hh of both LSTMs and W_ih of LSTM2 (what the decision looked at)
    float lstm_hh_norm = 0.f;        // max abs row sum of W_hh (reported, not decided on: ordinary LSTMs reach ~6)
    const char *precision = "fp16x3";  // "fp16x3" | "fp32-forced" (C3HIP_FP32=1) | "fp32-auto" (this decision) | "fp32-range-guard" | "fp32-verify" (verify mode escalated)

    // ---- switches (README) ----
    bool spp_fused = true;    // PyramidPolling as the epilogue of res3b (c3_conv3.h SPPF; 12 x 5 windows); env C3HIP_SPP_FUSED
    int wino = 2;             // stride-1 convolutions on F(2,3) along H (c3_conv3w.h: 12 instead of 18 piece-product groups per output pair)
                              // where the layer is a plain plane-to-plane one (res2a, res2b, res3a); env C3HIP_WINO: 0 = the direct kernels
                              // everywhere, 1 = only the 64- / 128-channel layers
    bool conv1_fused = true;  // conv1 computed inside res1a / res1b (c3_conv3.h SRC8): no conv1 launch, no conv1 planes; env C3HIP_CONV1_FUSED
    bool half_tiles = true;   // LSTM recurrences on 8-window tiles while 16-window tiles would leave CUs without a workgroup; env C3HIP_HALF_TILES
    int sharing = 1;          // handles the CALLER says feed this GPU side by side (c3_model_set_sharing): beside other batches the chip is
                              // full, so the recurrences stay on full tiles and the projection launches half as many, twice as long workgroups
    // a batch of the ring that runs in a lane NEXT TO another batch of the same handle (c3_hostring.h predict_submit) is in the same position
    // as one beside another handle: its recurrences take full 16-window tiles (128 workgroups per 1024 windows, so that two batches fill the 256
    // CUs between them -- a half-tile launch alone owns every CU: 144 KB of LDS per workgroup, and the second lane's batch waits), the
    // LSTM2 projection half its grid (profiles/r06_n_ab_lane_sharing.txt).  Set around forward_device by the ring; 1 everywhere else.
    int lane_sharing = 1;
    bool lane_beside = false;   // ... and whether any batch is in flight in another lane at all (run_tail's choice of full alignment's FC chain)
    unsigned lane_next = 0;     // the lane of the ring's next small batch (round robin over the submits)
    // As few streams as the work needs.  The runtime gives a process FOUR hardware queues (GPU_MAX_HW_QUEUES) and places every stream on the
    // least-used one; two streams on one queue run in submission order, and a wait between streams on two queues costs tens of microseconds.
    // Which streams meet on a queue depends on everything else the process created before -- measured (profiles/r06_o_*): the same ring of
    // 256-window batches ran at 650 k windows/s on the first handle of a fresh process and at 800 k on a second one, 620 k with 8 or 16 queues
    // (every stream alone: every dependency crosses queues).  So a small batch of the ring lives on its lane's stream ALONE -- staged windows in,
    // kernels, FC chain, rows out, in order, no event (the batches of the other lanes are what its copy runs under) -- and the transfer stream
    // exists only from the first batch on that stages outside a lane: three lanes + the null stream are the four queues.  (The FC chain on a
    // stream of its own gained 1.5 - 2 % in one placement of the streams and lost in another: profiles/r06_h_ab_tail_stream.txt, r06_o_*.)
    bool tail_fused = false;  // the split-K sum of L4 inside fc_tail_mfma_kernel (c3_tail.h) instead of its own launch: on for the pileup network (+0.7 %:
                              // 15 partials of 128 features), off for full alignment (-1 %: four branch workgroups re-read 28 partials of 256
                              // on a 64-workgroup grid), which takes fa_tail's kernel below instead
    // Full alignment has a two-launch chain of its own (c3_tail.h fc_tail_sum_kernel<W>: W windows per workgroup, every partial of an item in
    // flight at once).  env C3HIP_FA_TAIL = auto | split | w4 | w8 | w16: 0 = auto (run_tail: the smallest W whose grid has no more workgroups
    // than the device has CUs, the three launches beyond fa_tail_max_batch windows and beside other batches), -1 = split (the three
    // launches), 4 / 8 / 16 = that W whatever the batch.  The fp32 forms and the pileup network do not look at it.
    // Beside other batches -- the caller's sharing hint, or a batch in flight in another lane of the ring -- auto stays on the three launches:
    // a 512-thread workgroup with 229 registers per lane starts only on a CU that holds nothing else, and behind the convolution
    // workgroups of the neighbours it waits for one (three batches in flight, B = 256: 867 k -> 854 k windows/s with the fused form)
    int fa_tail = 0;
    // 512: with four branches that is the last batch W = 8 covers with one workgroup per CU.  Measured (profiles/fa_tail_two_launches.txt,
    // forms alternating in one process): the chain's two launches 3.4 us shorter at 256 windows (w4) and 2.9 us at 512 (w8), but W = 16 no
    // better than the three launches at 512 and 6.6 us longer at 1000, where its workgroups sum two items one after the other
    int64_t fa_tail_max_batch = 512;
    // Wave priority between the two workgroups of a CU (c3_conv3.h wave_prio_masks; DESIGN.md 3.8-10, profiles/wave_priority.txt): the schemes
    // run_fa_planes gives the convolution kernels, and only while the handle has the chip to itself -- beside other handles or lanes a
    // workgroup's CU mate is somebody else's.  env C3HIP_WAVE_PRIO = 0 | 1, read when the handle is created; rows do not depend on it
    bool wave_prio = true;
    int wg_slots = 512;       // co-resident 256-thread / 64 KiB-LDS workgroups on the device (2 per CU)

    // the reference's rescaling of very deep pileup windows (c3_rescale.h; the *_depth entries and c3_predict_submit_region)
    int max_depth = 144;   // shared/param_p.py:15 max_depth_dict: 144 on every platform (c3_model_set_max_depth)
    int64_t rescaled = 0;  // windows rescaled in the last call (c3_model_describe)
    int64_t cand_n = 0, cand_kept = 0, cand_chunks = 0;  // of the last candidate call that completed (c3_model_describe)
    // full-alignment windows as occupied rows (c3_expand.h)
    bool pack_rows = false;  // env C3HIP_PACK_ROWS=1: c3_predict / c3_predict_submit pack int8 windows while they stage them
    int64_t rows_windows = 0, rows_shipped = 0;  // windows that travelled as rows in the last completed call, and their rows (c3_model_describe)
    bool rows_call = false;  // inside a c3_predict that runs its batch as pieces: the two counts add up over the pieces

    // ---- verify mode (c3_model_set_verify, c3_verify.h): off = nothing allocated, nothing launched ----
    int verify_every = 0;  // every n-th submit of the ring also runs on the fp32 forms and is compared; 0 = off
    float verify_tol = 1e-4f, verify_near_tie = 1e-6f;
    int verify_policy = C3_VERIFY_REPORT;
    bool verify_seen = false;  // verify mode is or was on: c3_model_describe ends on verify=...
    int verify_ref = C3_VERIFY_REF_FP32;  // c3_model_set_verify_reference: what a selected batch is compared with
    c3_verify_extra vextra = {};          // the totals that c3_verify_stats has no room for (reference is filled in when read)
    bool answer_exact = false;            // c3_model_set_answer(C3_ANSWER_EXACT): every batch of the ring is answered by the exact form
    c3_verify_stats vstats = {};  // totals since the last load / reset (batches_submitted doubles as the selection counter)
    // ... layer records (c3_model_set_verify_layers): off = nothing allocated, nothing launched, a verified batch laid out as without it
    bool verify_layers = false;
    bool verify_layers_seen = false;         // is or was on: c3_model_verify_layers lists the layers
    c3_verify_layer vlayer[kLayerMaxLayers] = {};  // totals per layer in network order since the last load / reset
    int64_t vlayer_batches = 0;              // batches that brought layer records
    int *layer_exp = nullptr;                // device [9][256]: act_exp as the compare kernel reads it; uploaded on first use after a load
    bool layer_exp_ok = false;
    int layer_pass = 0;                      // forward_device is enqueuing 1: the product pass, 2: the fp32 pass of ...
    HostSlot *layer_slot = nullptr;          // ... this slot's batch with layer records
    int64_t layer_batch = 0;                 // ... of this many windows
    const uint32_t *layer_kept_count = nullptr;  // ... a candidate batch: the device word with its kept count

    // ---- score mode (c3_model_set_score, c3_score.h): off = nothing allocated, nothing launched ----
    bool score_on = false;
    double score_gamma = 2.0;
    bool score_weighted = false;
    float score_w[kScoreMaxCols] = {};  // class weights in the row's column layout
    // ... and its census (c3_model_set_score_census, c3_census.h): off = no section in a staged batch, nothing launched, nothing copied
    bool score_census_on = false, score_census_seen = false;  // seen: is or was on -- c3_score_census_read / _reset answer
    c3_score_census score_census = {};                        // totals of the completed batches since the last reset

    // ---- refine mode (c3_model_set_refine, c3_refine.h): off = no section in a staged batch, nothing allocated, launched or copied ----
    bool refine_on = false, refine_seen = false;  // seen: is or was on (the totals start with it)
    float refine_gap = 0.f;
    c3_refine_stats rfstats = {};     // totals since the last load / reset (gap is filled in when read)
    float *refine_rows = nullptr;     // device: the refined rows of the batch c3_predict_wait is completing; grown on demand, freed with the handle
    size_t refine_rows_bytes = 0;

    // ---- calibration (c3_calibrate.h; full alignment): off = nothing allocated, nothing launched, a load packs what it packs without it ----
    int census_pass = 0;              // forward_device is enqueuing a census pass: tap() takes the channels' maxima instead of copying
    uint32_t *census_dev = nullptr;   // device [9][256]: bit patterns of max |x| per convolution and channel, in the units of the current load
    float census[9][256] = {};        // the same in the checkpoint's units, accumulated over calls until c3_model_calibrate_reset
    int64_t census_windows = 0;
    bool lowering_set = false;        // c3_model_set_channel_lowering: the next loads pack k = k0 - lowering (survives a load, like the plan)
    uint8_t lowering[kCalChannels] = {};
    int lowering_cap = 0;             // ... and where that lowering came from, recorded WITH it (c3_model_describe): the cap and the windows of
    int64_t lowering_windows = 0;     //     the solve that made it (c3_model_set_calibration_origin for one made elsewhere; 0 = not known)
    bool solved = false;              // the handle's last c3_model_calibration_solve: its result, cap and the census windows it saw
    uint8_t solved_lowering[kCalChannels] = {};
    int solved_cap = 0;
    int64_t solved_windows = 0;
    bool chan_ok = false;             // a load has filled ...
    int8_t chan_k0[kCalChannels] = {}, chan_k[kCalChannels] = {};  // ... the exponents fa_channel_exps gave it / it runs with

    // ---- the range-guard policy (c3_model_set_range_policy; c3_calibrate.h range_guard_recalibrate): sticky = nothing kept, nothing counted ----
    int range_policy = C3_RANGE_STICKY;
    int range_max_recal = 0;
    c3_range_stats rstats = {};       // totals since the last load (census_windows, policy and max_recalibrations are filled in when read)
    uint64_t pack_epoch = 0;          // how often the weights of this load were packed again
    std::vector<KeptTensor> kept;     // RECALIBRATE: the float32 tensors of the last load, what a repack packs from

    ExactState exact;

    void *decode_dev = nullptr;  // scratch of c3_outcome_maxima
    size_t decode_bytes = 0;

    // ---- the variant instruments (jackknife, subsample and occlusion mode; c3_variants.h): never called = nothing allocated, nothing launched ----
    void *variant_dev = nullptr;  // a pass's staged input, its meta block, the rows of its dense windows, its records and drops / masks; grown on demand
    size_t variant_bytes = 0;

    // ---- workspaces and kernel streams: the lanes (Lane above; lane(m) is the active one) ----
    Lane lanes[kMaxLanes];
    int lane_cur = 0;
    int ring_lanes = 1;  // 1 .. kMaxLanes (set in c3_model_create: the kind's default, or env)
    int64_t lane_max_batch = 0;  // batches up to this many windows take the next lane, larger ones the first lane (env C3HIP_RING_LANES_MAX_BATCH)
    bool keep = false;  // debug: one buffer per layer instead of the 3-buffer rotation

    // ---- debug taps (c3_debug_tap): layer outputs of the forms a call really runs, each copied on its producing stream right behind
    // the producing launch into a buffer of the handle, at the window's position in the call (micro-batches, ring lanes) ----
    uint32_t tap_mask = 0;                                // bit per kTap* tensor; 0 = off: no copy, no allocation, the launches of an untapped call
    uint32_t tap_written = 0, tap_skipped = 0, tap_planes = 0;  // of the last call: copied / not produced by its form / held as planes
    float *tap_dev[kTapCount] = {};
    size_t tap_bytes[kTapCount] = {};
    int64_t tap_n = 0, tap_base = 0;  // windows of the last call; first window of the part being enqueued
    bool tap_call = false;            // inside a c3_predict that runs its batch as pieces: the taps are sized for the whole call
    int64_t tap_call_off = 0;         // ... and the piece being enqueued starts at this window of it

    HostSlot slot[kHostSlots];

    // which kernel forms the last forward pass took (c3_model_describe; bench.py reports it).  ONE struct: verify mode's second pass
    // (c3_hostring.h shadow_pass) puts it back as a whole, so whatever forward_device reports belongs in here
    struct Choices {
        const char *lstm1 = "-", *proj2 = "-", *lstm2 = "-", *fa = "-";
        const char *s2[2] = {"-", "-"};  // conv3, conv5: one or two workgroups per CU (c3_conv3s2.h PAIR)
        char s1[8] = "------";           // the six stride-1 convolutions res1a .. res3b: d = direct, w = F(2,3) along H
        char wform[8] = "------";        // ... and the form of the F(2,3) ones (c3_conv3w.h): p = paired workgroups, t = transform waves
        const char *fa_tail = "-";       // full alignment's FC chain (run_tail): split | fused-w4 | fused-w8 | fused-w16
        uint32_t prio = 0;               // bit l: convolution l of the full-alignment pass ran a wave priority scheme (c3_conv3.h wave_prio_masks)
    } choice;

    bool prof = false;
    std::vector<ProfRec> recs;
};

static int conv_out(int n, int s) { return (n - 1) / s + 1; }

// THE predicate of the plan: layer `bit` takes its product (fp16x3) form
static bool layer_f16(const c3_model *m, uint32_t bit) { return m->f16_ok && !((m->fp32_plan | m->fp32_auto) & bit); }

// the active lane: the workspace and the kernel stream of the forward pass being enqueued
static Lane &lane(c3_model *m) { return m->lanes[m->lane_cur]; }
// make lane k the active one; its kernel stream is created on first use (every stream of a handle: non-blocking, default priority)
static int use_lane(c3_model *m, int k) {
    if (k < 0 || k >= kMaxLanes) return fail("lane %d out of range", k);
    m->lane_cur = k;
    if (!m->lanes[k].stream) HIP_TRY(hipStreamCreateWithFlags(&m->lanes[k].stream, hipStreamNonBlocking));
    return 0;
}

static void fa_geometry(const c3_model *m, int hh[10], int ww[10]) {
    hh[0] = m->depth, ww[0] = m->positions;
    for (int l = 0; l < 9; ++l) hh[l + 1] = conv_out(hh[l], kConvStride[l]), ww[l + 1] = conv_out(ww[l], kConvStride[l]);
}

// ------------------------------------------------------------------------------------------ profiling scope
// dense MFMA peaks of MI355X (MI355X_MICROARCH.md): v_mfma_f32_32x32x16_f16 / 16x16x32_f16 and the fp32-input forms
static constexpr double kPeakF16 = 2500.0, kPeakF32 = 157.3;
struct ProfScope {
    c3_model *m;
    hipStream_t s;
    ProfRec r;
    bool on;
    ProfScope(c3_model *m_, hipStream_t s_, const char *name, double flops, double bytes) : m(m_), s(s_), on(m_->prof) {
        if (!on) return;
        r.name = name, r.flops = flops, r.bytes = bytes;
        (void)hipEventCreate(&r.a);
        (void)hipEventCreate(&r.b);
        (void)hipEventRecord(r.a, s);
    }
    // executed matrix work of the launch and the roof of the instruction it uses (c3_kernel_stat.mfma_flops / mfma_peak_tflops)
    void mfma(double flops, bool f16) { r.mfma_flops = flops, r.mfma_peak = f16 ? kPeakF16 : kPeakF32; }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(r.b, s);
        m->recs.push_back(r);
    }
};

// ------------------------------------------------------------------------------------------ launches
template <class Loader, int EPI, int BM, int BN, int SPLIT = 0>
static int launch_gemm(hipStream_t s, const typename Loader::Params &lp, const float *bt, int64_t ldb, int M, int N,
                       int nk, int splits, const EpilogueParams &ep, const float *bt16 = nullptr) {
    if (N % BN) return fail("internal: N=%d not a multiple of BN=%d", N, BN);
    if (M <= 0) return 0;
    GemmParams gp;
    gp.bt = bt, gp.ldb = ldb, gp.M = M, gp.N = N, gp.nk = nk;
    gp.bt3 = reinterpret_cast<const uint16_t *>(bt16);
    gp.tiles_n = N / BN;
    gp.tiles = ((M + BM - 1) / BM) * gp.tiles_n;
    dim3 grid(gp.tiles, splits);
    hipLaunchKernelGGL((gemm_mfma_kernel<Loader, EPI, BM, BN, SPLIT>), grid, dim3(kThreads), 0, s, lp, gp, ep);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Split-K factor of the L4 GEMM (K = 10560 / 3584, N = 128 / 256: far too few output tiles to fill 256 CUs).
// It is a constant of the model, NOT a function of the batch size: the partial sums are added in a fixed
// order by the reduce kernel, so a window's probabilities are bit-identical whatever batch it travels in.
static int l4_splits(const c3_model *m) {
    const int nk = m->K4 % 64 == 0 ? m->K4 / 64 : m->K4 / kBK;  // l4_stream_kernel (c3_l4.h) walks chunks of 64 inputs, the fp32 form chunks of kBK
    const int want = m->kind == C3_KIND_PILEUP ? 15 : 28;  // measured against 22 / 30 / 33 (pileup) and 14 / 56 (full alignment)
    int best = 1;
    for (int s = 1; s <= nk && s <= want; ++s)
        if (nk % s == 0) best = s;
    return best;
}

// ------------------------------------------------------------------------------------------ memory
static int dev_alloc(Lane &L, void **p, size_t bytes) {
    DevBuf b;
    b.bytes = bytes;
    HIP_TRY(hipMalloc(&b.p, std::max<size_t>(bytes, 256)));
    L.bufs.push_back(b);
    *p = b.p;
    return 0;
}
// ---- PAGEABLE host memory never meets the device directly.  A hipMemcpy from (or to) pageable memory makes the runtime pin the
// caller's pages, and it keeps them registered with the device for as long as the range stays mapped (measured, tools/
// fork_stall_probe.hip: after a 256 MB pageable upload the first kernel behind a fork() completes 3.3 s late -- fork write-protects
// the registered pages, the driver evicts the process's queues and revalidates every registered page; with the source freed, or with
// no pageable copy at all, nothing happens).  The reference's stage-B loop forks its decode pool right after its first model call
// (clair3/CallVariantsFromCffi.py:302): with the weights uploaded from the state dict's pageable arrays that fork cost ~0.3 s of
// every run of the loop (tests/diag/fork_stall.py: first call after the forks 320 ms, then 2.8 ms).  So every such copy goes through
// ONE pinned bounce buffer that forked children do not inherit.
// Handles must not be used in a forked child: their pinned buffers are not there (MADV_DONTFORK) and a touch faults.
static void keep_out_of_children(void *p, size_t bytes) {  // (what ibv_fork_init does for RDMA buffers; a child could not use the handle anyway)
    if (!p || !bytes) return;
    // madvise works on whole pages: every caller allocates page-multiples with hipHostMalloc (page-aligned, page-exclusive); anything
    // else would take a neighbour's bytes out of the children too, so it is refused here and said once
    static std::atomic<bool> said{false};
    if (((uintptr_t)p & 4095) != 0 || (bytes & 4095) != 0) {
        if (!said.exchange(true)) fprintf(stderr, "libc3hip: a pinned buffer of %zu bytes at %p is not page-granular: left visible to forked children\n", bytes, p);
        return;
    }
    if (madvise(p, bytes, MADV_DONTFORK) != 0 && !said.exchange(true))
        fprintf(stderr, "libc3hip: madvise(MADV_DONTFORK) failed (%s): pinned staging memory stays visible to forked children (a fork then stalls the device longer)\n", strerror(errno));
}
// One bounce buffer PER DEVICE, each with its own lock (round 5 had one for the process: weight uploads, c3_outcome_maxima and
// c3_decode_columns of handles on different GPUs serialised on it), portable (usable by every device's copies whatever device was
// current when it was made), in two halves: the host memcpy of chunk i + 1 runs under the DMA of chunk i.
struct BounceBuf {
    static constexpr size_t kBytes = (size_t)8 << 20, kHalf = kBytes / 2;
    std::mutex mu;
    void *pin = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
};
static BounceBuf &bounce_buf() {
    constexpr int kMaxDev = 64;
    static BounceBuf *b = new BounceBuf[kMaxDev];  // never destroyed (handles may outlive static destruction at exit)
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= kMaxDev) d = 0;
    return b[d];
}
static int bounce_ready(BounceBuf &b) {
    if (!b.pin) {
        HIP_TRY(hipHostMalloc(&b.pin, BounceBuf::kBytes, hipHostMallocPortable));
        keep_out_of_children(b.pin, BounceBuf::kBytes);
        for (hipEvent_t &e : b.ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    return 0;
}
// dev[0, bytes) = src[0, bytes): synchronous (src may be reused on return); s orders the copy behind the stream's work.  The device
// whose buffer is used is the CURRENT one: every caller has made the handle's device current (hipSetDevice) before it gets here.
static int h2d_staged(void *dev, const void *src, size_t bytes, hipStream_t s = nullptr) {
    BounceBuf &b = bounce_buf();
    std::lock_guard<std::mutex> lk(b.mu);
    TRY(bounce_ready(b));
    int i = 0;
    for (size_t off = 0; off < bytes; off += BounceBuf::kHalf, ++i) {
        const size_t n = std::min(BounceBuf::kHalf, bytes - off);
        char *half = (char *)b.pin + (i & 1) * BounceBuf::kHalf;
        if (i >= 2) HIP_TRY(hipEventSynchronize(b.ev[i & 1]));  // the DMA that read this half two chunks ago
        memcpy(half, (const char *)src + off, n);
        HIP_TRY(hipMemcpyAsync((char *)dev + off, half, n, hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(b.ev[i & 1], s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}
// dst[0, bytes) = dev[0, bytes) behind the stream's work: synchronous
static int d2h_staged(void *dst, const void *dev, size_t bytes, hipStream_t s = nullptr) {
    BounceBuf &b = bounce_buf();
    std::lock_guard<std::mutex> lk(b.mu);
    TRY(bounce_ready(b));
    int i = 0;
    size_t prev_off = 0, prev_n = 0;
    for (size_t off = 0; off < bytes; off += BounceBuf::kHalf, ++i) {
        const size_t n = std::min(BounceBuf::kHalf, bytes - off);
        char *half = (char *)b.pin + (i & 1) * BounceBuf::kHalf;
        HIP_TRY(hipMemcpyAsync(half, (const char *)dev + off, n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(b.ev[i & 1], s));
        if (i >= 1) {  // chunk i - 1 leaves the other half while chunk i arrives
            HIP_TRY(hipEventSynchronize(b.ev[(i - 1) & 1]));
            memcpy((char *)dst + prev_off, (char *)b.pin + ((i - 1) & 1) * BounceBuf::kHalf, prev_n);
        }
        prev_off = off, prev_n = n;
    }
    if (i >= 1) {
        HIP_TRY(hipEventSynchronize(b.ev[(i - 1) & 1]));
        memcpy((char *)dst + prev_off, (char *)b.pin + ((i - 1) & 1) * BounceBuf::kHalf, prev_n);
    }
    return 0;
}

static int upload(c3_model *m, float **dst, const std::vector<float> &src) {
    void *p = nullptr;
    HIP_TRY(hipMalloc(&p, std::max<size_t>(src.size() * sizeof(float), 256)));
    TRY(h2d_staged(p, src.data(), src.size() * sizeof(float)));
    if (*dst) (void)hipFree(*dst);
    *dst = (float *)p;
    (void)m;
    return 0;
}

static void free_workspace(Lane &L) {
    for (auto &b : L.bufs) (void)hipFree(b.p);
    L.bufs.clear();
    L.cap = 0;
    if (L.xr) (void)hipFree(L.xr);
    L.xr = nullptr, L.xr_cap = 0;
    if (L.xe) (void)hipFree(L.xe);
    L.xe = nullptr, L.xe_cap = 0;
    if (L.xo) (void)hipFree(L.xo);
    L.xo = nullptr, L.xo_cap = 0;
}
static void free_all_workspaces(c3_model *m) {  // every lane's (geometry change, destruction)
    for (Lane &L : m->lanes) free_workspace(L);
}

static void exact_free_workspace(c3_model *m) {  // (geometry change, growth, destruction)
    ExactState &E = m->exact;
    for (void *p : E.ws) (void)hipFree(p);
    E.ws.clear();
    E.cap = 0, E.x_window_bytes = 0, E.last_n = 0;
}
static void exact_free_weights(c3_model *m) {
    for (void *p : m->exact.weights) (void)hipFree(p);
    m->exact.weights.clear();
    m->exact.loaded = false, m->exact.last_n = 0;
}

static int64_t max_microbatch(const c3_model *m) { return m->kind == C3_KIND_PILEUP ? 16384 : 2048; }

static int ensure_workspace(c3_model *m, int64_t n) {  // the active lane's
    Lane &L = lane(m);
    n = std::min<int64_t>(n, max_microbatch(m));
    if (n <= L.cap) return 0;
    HIP_TRY(hipDeviceSynchronize());
    free_workspace(L);
    if (m->kind == C3_KIND_FULL_ALIGNMENT) {
        int hh[10], ww[10];
        fa_geometry(m, hh, ww);
        size_t act_elems[9];
        size_t biggest = 0;
        for (int l = 0; l < 9; ++l) {
            act_elems[l] = (size_t)hh[l + 1] * ww[l + 1] * kConvCout[l];
            biggest = std::max(biggest, act_elems[l]);
        }
        if (m->keep) {
            for (int l = 0; l < 9; ++l) TRY(dev_alloc(L, (void **)&L.act[l], act_elems[l] * n * sizeof(float)));
        } else {
            float *rot[3];
            for (int i = 0; i < 3; ++i) TRY(dev_alloc(L, (void **)&rot[i], biggest * n * sizeof(float)));
            for (int l = 0; l < 9; ++l) L.act[l] = rot[l % 3];
        }
        TRY(dev_alloc(L, (void **)&L.spp, (size_t)n * m->K4 * sizeof(float)));
    } else {
        const int T = m->positions;
        TRY(dev_alloc(L, (void **)&L.h1, (size_t)n * T * 256 * sizeof(float)));
        TRY(dev_alloc(L, (void **)&L.gx2, (size_t)n * T * 1280 * sizeof(float)));
        TRY(dev_alloc(L, (void **)&L.h2, (size_t)n * T * 320 * sizeof(float)));
    }
    TRY(dev_alloc(L, (void **)&L.part, (size_t)l4_splits(m) * n * m->FC * sizeof(float)));  // [S][n][FC]
    TRY(dev_alloc(L, (void **)&L.l4dbg, (size_t)n * m->FC * sizeof(float)));
    L.cap = n;
    return 0;
}

// the active lane's buffer of rescaled windows (c3_rescale.h), as many as its workspace holds; only a handle that is given depths has one
static int ensure_rescale_buf(c3_model *m) {
    Lane &L = lane(m);
    if (L.xr && L.xr_cap >= L.cap) return 0;
    HIP_TRY(hipDeviceSynchronize());  // (a batch in flight in this lane may still read the smaller one)
    if (L.xr) (void)hipFree(L.xr);
    L.xr = nullptr, L.xr_cap = 0;
    HIP_TRY(hipMalloc((void **)&L.xr, std::max<size_t>((size_t)L.cap * m->positions * m->C * sizeof(int32_t), 256)));
    L.xr_cap = L.cap;
    return 0;
}

// the active lane's buffer of expanded full-alignment windows (c3_expand.h), as many as its workspace holds (2048 windows x 23.5 KB = 48 MB
// at most); only a handle that is given rows has one
static int ensure_expand_buf(c3_model *m) {
    Lane &L = lane(m);
    if (L.xe && L.xe_cap >= L.cap) return 0;
    HIP_TRY(hipDeviceSynchronize());  // (a batch in flight in this lane may still read the smaller one)
    if (L.xe) (void)hipFree(L.xe);
    L.xe = nullptr, L.xe_cap = 0;
    HIP_TRY(hipMalloc((void **)&L.xe, std::max<size_t>((size_t)L.cap * m->depth * m->positions * m->C, 256)));
    L.xe_cap = L.cap;
    return 0;
}
