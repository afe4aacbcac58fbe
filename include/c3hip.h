/*
 * c3hip.h -- C ABI of libc3hip.so, the MI355X (gfx950) native inference path for the two Clair3
 * networks.  This is the drop-in boundary for the *model call* of the reference's
 * CallVariantsFromCffi / CallVariantsFromCffiGPU step; everything else of the reference pipeline
 * (tensor extraction, VCF emitters, run_clair3.py) stays untouched.
 *
 * What each entry point replaces in the reference (paths relative to the Clair3 repo):
 *
 *   c3_device_count / c3_mem_info   nvidia-smi parsing in clair3/CallVariantsFromCffiGPU.py:13-43
 *                                   (get_gpu_memory / check_gpu_memory) -- not available on ROCm.
 *   c3_model_create                 model factory  clair3/CallVariantsFromCffi.py:223-243
 *                                   (Clair3_P / Clair3_F(add_indel_length, predict=True, input_channels)),
 *                                   clair3/model.py:58-128 and :282-368; device selection :215-221.
 *   c3_model_load                   _load_torch_checkpoint + strict load_state_dict,
 *                                   clair3/CallVariantsFromCffi.py:19-28 (the Python wrapper does the
 *                                   torch.load and hands the named float32 tensors over).
 *   c3_predict                      _torch_predict(model, device, X) -> numpy (B, 24|90) float32,
 *                                   clair3/CallVariantsFromCffi.py:48-52 (twin: clair3/CallVariants.py:83-87):
 *                                   H2D copy + Clair3_P.forward (model.py:130-161) or Clair3_F.forward
 *                                   (model.py:377-416) + D2H copy.
 *   c3_predict_submit / _wait       same, split so the caller's loop (CallVariantsFromCffi.py:302-353)
 *                                   can overlap batch i+1's transfer with batch i's kernels/decoding.
 *   c3_predict_device               the forward pass alone on tensors already resident in HBM
 *                                   (what bench.py times; also the hook for the RCCL gather of SURVEY 8e).
 *   c3_model_destroy                model going out of scope at process exit.
 *   c3_vcf_rows                     the per-row Python of the decoder: batch_output -> output_with -> output_from with its allele
 *                                   lookups (clair3/CallVariants.py:1069-1394, :676-1016, :117-201, :662-673) for rows that carry the
 *                                   decoder columns -- one pass of plain host code per batch.
 *   c3_predict_pileup_candidates    the loop that slices a region's pileup into windows, preprocess/CreateTensorPileupFromCffi.py:343-397
 *                                   with __enforce_pileup_chunk_contiguity :180-236 (chunk lookup, offsets, the empty-column test, head /
 *                                   tail padding), followed by the model call: candidate positions in, rows and statuses out.
 *   c3_predict_rows / _submit_rows  the zero rows of a full-alignment window: the stream format carries the reads' rows only and the generator
 *                                   pads them to the matrix depth on the host before the model call, clair3/utils.py:113-121 (its C producer
 *                                   lays the dense matrix out by the same rule, src/clair3_full_alignment_dwell.c:139-150): rows in, padded on
 *                                   the device.
 *   c3_device_pci_bus_id            where a GPU slot's worker belongs on the host (the reference leaves placement to the OS,
 *                                   clair3/CallVariantsFromCffiGPU.py:138-156).
 *
 * Conventions (mirroring libclair3's cffi surface, build.py:38-85, src/clair3_pileup.h:90-113):
 *   - plain C types only; the library owns all device memory; the caller owns host x / y buffers
 *     (C-contiguous; pageable is fine -- the library stages through its own pinned buffers);
 *   - every int-returning function returns 0 on success, non-zero on failure, and c3_last_error()
 *     then describes the failure (thread-local).  Nothing aborts the process;
 *   - one model per handle, one handle per OS process per GPU slot is the intended use
 *     (clair3/CallVariantsFromCffiGPU.py:163-199 launches one worker per slot); a handle is not
 *     thread-safe, different handles are independent.
 *   - the output row layout is exactly the reference's: [gt21 (21) | genotype (3) | indel_1 (33) |
 *     indel_2 (33)], columns label_shape_cum = 21,24,57,90 (shared/param_p.py:37-39), float32
 *     probabilities, consumed unchanged by batch_output (clair3/CallVariants.py:1069-1116).
 */
#ifndef C3HIP_H
#define C3HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define C3_KIND_PILEUP 0         /* Clair3_P, windows (B, 33, C)    int8 | int32 */
#define C3_KIND_FULL_ALIGNMENT 1 /* Clair3_F, windows (B, D, 33, C) int8, channels-last */

#define C3_DTYPE_I8 0
#define C3_DTYPE_I32 1
#define C3_DTYPE_F32 2
#define C3_DTYPE_I64 3

typedef struct c3_model c3_model;

/* one entry of a PyTorch state_dict */
typedef struct {
    const char *name;  /* e.g. "LSTM1.weight_ih_l0", "conv1.bn.running_var" */
    int32_t dtype;     /* C3_DTYPE_F32 for every parameter/buffer; *.num_batches_tracked (I64) is accepted and ignored */
    int32_t ndim;
    int64_t shape[4];
    const void *data;  /* host pointer, C-contiguous */
} c3_tensor_desc;

const char *c3_version(void);
/* thread-local description of the last failure in this thread ("" if none) */
const char *c3_last_error(void);

/* number of visible HIP devices (honours HIP_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES); <0 on error */
int c3_device_count(void);
int c3_mem_info(int device, size_t *free_bytes, size_t *total_bytes);
/* PCI address of a visible device as sysfs spells it ("0000:c5:00.0"): /sys/bus/pci/devices/<address>/numa_node is the NUMA
 * node the host side of a rank -- staging copies, the forked decode workers -- belongs on (clair3_amd/dist.py pin_to_device_numa).
 * The reference starts one worker process per GPU slot and leaves placement to the OS (clair3/CallVariantsFromCffiGPU.py:138-156,
 * parallel -j); SURVEY 8e names NUMA placement as a limiter of the 1 -> 8 GPU scaling. */
int c3_device_pci_bus_id(int device, char *buf, int buf_bytes);

/* kind: C3_KIND_*; in_channels: 18 (pileup) / 8 or 9 (full alignment, 9 = dwell time);
 * add_indel_length: 0 -> (B,24) output, 1 -> (B,90).  Returns NULL on failure. */
c3_model *c3_model_create(int kind, int in_channels, int add_indel_length, int device);
/* window geometry; defaults are the ONT shapes: depth 89 (ignored for pileup), 33 positions.  A change frees the workspaces and
 * drops the weights (load again); the geometry the handle already has changes nothing.  Refused, with nothing touched, while a
 * c3_predict_submit of the handle is pending. */
int c3_model_set_geometry(c3_model *m, int depth, int positions);
/* strict: every expected key must be present with the expected shape, unknown keys are an error.  A (re)load starts
 * the handle afresh: the range guard's flag is cleared and the precision goes back to what C3HIP_FP32 chose, else to
 * the load-time decision (pileup) or fp16x3.  Refused while a c3_predict_submit of the handle is pending. */
int c3_model_load(c3_model *m, const c3_tensor_desc *tensors, int n_tensors);
/* 24 or 90 */
int c3_model_output_size(const c3_model *m);
/* Decoder columns: with enable != 0 every output row of c3_predict / c3_predict_submit /
 * c3_predict_device / c3_predict_pileup_region grows from c3_model_output_size() to c3_model_row_size() =
 * output_size + C3_DECODE_COLS floats.  The caller of _torch_predict (clair3/CallVariantsFromCffi.py:48-52, :317)
 * does not know the reference base of a row, so the columns carry what clair3/CallVariants.py:510-659 + :722-749
 * derive from the row for EVERY base (same float32 products, same order as c3_outcome_maxima):
 *   [0..8]   max of the class lists homo_SNP, hetero_SNP, homo_Ins, homo_Del, hetero_ACGT_Ins, hetero_InsIns,
 *            hetero_ACGT_Del, hetero_DelDel, hetero_InsDel        [9..12] homo_Ref probability if the base is A, C, G, T
 *   [13..21] position of the first occurrence of each maximum     [22]    bit b set: base b takes the early exit
 *   [23..26] the class output_from settles on first (:722-751) if the base is A, C, G, T: 0 = homo_Ref (the overall maximum, or
 *            the early exit), else the first class of its if / elif chain (:753-978) whose list holds the overall maximum
 *   [27..30] 100 x QUAL of that first decision (quality_score_from, :375-381), an integer: QUAL = column / 100.0
 * (positions, classes, bits and 100 x QUAL stored as float values).  Rows stay valid input of the reference's batch_output: it slices
 * columns [0:21] [21:24] [24:57] [57:90] (CallVariants.py:1072-1080) and never looks further right. */
#define C3_DECODE_COLS 31
int c3_model_set_decode_columns(c3_model *m, int enable);
int c3_model_row_size(const c3_model *m);
/* bytes of one input window for dtype x_dtype (594 / 2376 / 23496 / 26433 for the ONT shapes) */
int64_t c3_model_window_bytes(const c3_model *m, int x_dtype);

/* y_host[batch][24|90 (c3_model_row_size)] = forward(x_host[batch][...]); synchronous.  A batch of two or more chunks (256
 * full-alignment / 4096 pileup windows) travels through slots 0..2 of the submit / wait ring below in growing pieces:
 * no c3_predict_submit of this handle may be pending on those slots. */
int c3_predict(c3_model *m, const void *x_host, int x_dtype, int64_t batch, float *y_host);
/* Note on the arithmetic: the contractions form their fp32 products from two fp16 pieces per operand (fp16x3, DESIGN.md 1:
 * fp32-level parity).  Should a checkpoint ever drive an activation towards the fp16 range (|x| >= 16000), c3_predict /
 * c3_predict_wait notice (a flag raised by the kernels, or a non-finite row), print one line to stderr, switch the handle
 * to the fp32 matrix instructions for the rest of its life and run the batch again; c3_predict_device does not check
 * (c3_predict_device_checked does; c3_model_range_status reports). */
#define C3_HOST_SLOTS 4
/* asynchronous pair, slot in [0, C3_HOST_SLOTS): submit copies x into pinned staging and enqueues H2D + kernels + D2H;
 * wait blocks until y_host of that slot is complete. x_host may be reused as soon as submit returns.  Batches in different slots
 * may run side by side on the device (the handle keeps up to three lanes -- workspace + kernel stream -- for batches that do not fill the
 * chip by themselves; C3HIP_RING_LANES): rows never depend on the slot, the lane or the batch a window travels in. */
int c3_predict_submit(c3_model *m, const void *x_host, int x_dtype, int64_t batch, float *y_host, int slot);
int c3_predict_wait(c3_model *m, int slot);
/* The same ring with the rows LEFT ON THE DEVICE: y_dev is a device pointer on the model's device (batch x c3_model_row_size()
 * floats) that the forward pass writes directly; nothing but the range flag crosses PCIe on the way out.  For a rank of a
 * sharded job whose rows go to c3_gather_rows, not to its own host -- the reference's per-GPU workers each write their rows to
 * disk (clair3/CallVariantsFromCffiGPU.py:138-199); here they meet on rank 0 over xGMI and cross PCIe once, there.
 * c3_predict_wait(slot) runs the range guard (flag + a device-side scan for non-finite rows) and re-runs on fp32 if needed. */
int c3_predict_submit_dev(c3_model *m, const void *x_host, int x_dtype, int64_t batch, float *y_dev, int slot);
/* ---- one batch staged from SEVERAL host buffers (clair3_amd/serve.py: one GPU process answering the reference's CPU workers) ----
 * The reference's authors let the per-chunk CPU workers of `parallel ... CallVariantsFromCffi` send their batches to one GPU process
 * (--use_triton_gpu, clair3/CallVariantsFromCffi.py:201-214,287-294: models `pileup` INT32 and `alignment` INT8).  A server that coalesces the
 * requests of several clients needs one forward pass over windows that sit in several buffers:
 *   parts[i]    counts[i] windows (C-contiguous, c3_model_window_bytes(x_dtype) each); y_parts[i]: where their counts[i] rows of
 *               c3_model_row_size() floats go (decoder columns included).  1 <= n_parts <= C3_MAX_PARTS; counts[i] == 0 is legal (its
 *               pointers are not read); all parts share x_dtype.  Windows only: pileup C3_DTYPE_I8 | C3_DTYPE_I32, full alignment
 *               C3_DTYPE_I8 -- depths, regions, candidates and rows keep their own entries
 *   meaning     part i is staged behind part i - 1 (the one copy every caller buffer gets), and from there on the batch IS the plain batch
 *               of sum(counts) windows c3_predict_submit takes: same lanes, range guard (its re-run works from the staged image; either
 *               policy), verify mode.  Rows are bit-identical to c3_predict on the concatenation, and so to c3_predict on each part alone
 *   errors      before anything is queued, the slot left free: n_parts outside [1, C3_MAX_PARTS], null tables, a negative count, a null
 *               buffer of a part with windows, a dtype the kind does not take, a busy slot
 * parts, counts, y_parts and every parts[i] may be reused as soon as submit returns; c3_predict_wait(slot) writes every y_parts[i].
 * c3_predict_parts = submit + wait on slot 0. */
#define C3_MAX_PARTS 64
int c3_predict_submit_parts(c3_model *m, const void *const *parts, const int64_t *counts, int n_parts, int x_dtype, float *const *y_parts,
                            int slot);
int c3_predict_parts(c3_model *m, const void *const *parts, const int64_t *counts, int n_parts, int x_dtype, float *const *y_parts);
/* There is deliberately NO entry that page-locks caller memory.  Rounds 3-5 exported c3_host_register /
 * c3_host_unregister / c3_model_set_lock_sources (hipHostRegister on a whole np.load'ed tensor file or on libclair3's
 * fa_data.matrix buffer, preprocess/CreateTensorFullAlignmentFromCffi.py:136-168).  On ROCm 7.2 a process that registers and
 * unregisters host ranges while ANOTHER HIP user in it (PyTorch) copies from pageable memory dies with "Memory access fault
 * by GPU" sooner or later (tests/diag/register_vs_torch_probe.py shows it with hipHostRegister and torch alone), and a C ABI
 * cannot see who shares its process: the entries were retired in round 6.  A foreign buffer -- numpy, a memory-mapped tensor
 * file, libclair3's matrix -- is handed to c3_predict / c3_predict_submit as it is and staged through the library's own
 * pinned memory (kept out of forked children); x_host may be reused as soon as the call returns. */
/* device-resident forward: x_dev / y_dev are device pointers on the model's device, stream is a
 * hipStream_t (NULL = the HIP null stream, i.e. PyTorch's default stream).  Asynchronous with respect to the
 * host; ordered like any other work on that stream.  Calls on one handle must not overlap each other (one
 * workspace per handle): keep several batches in flight with several handles.  x_dev may start at any byte address
 * (a slice of a larger tensor, an odd base for 9-channel windows) and y_dev at any float: the kernels read no byte
 * outside the batch*c3_model_window_bytes() window bytes and write no float outside the batch*c3_model_row_size() rows
 * (tests/test_caller_inputs_gpu.py). */
int c3_predict_device(c3_model *m, const void *x_dev, int x_dtype, int64_t batch, float *y_dev, void *stream);
/* The same forward with the range guard of c3_predict_wait (the device-resident entry a sharded job uses,
 * clair3_amd/dist.py): after the kernels it scans the rows for non-finite values on the device, reads the range flag,
 * and -- should either be raised -- switches the handle to the fp32 matrix instructions and runs the batch again.
 * Synchronises `stream` before returning (that is the price of the check; c3_predict_device stays asynchronous). */
int c3_predict_device_checked(c3_model *m, const void *x_dev, int x_dtype, int64_t batch, float *y_dev, void *stream);
/* For callers of the unchecked entry: *flag_out != 0 when any fp16x3 batch of this handle raised the range flag
 * (bit 0: a convolution output reached 16000, bit 1: a non-finite row seen by the checked entry), *on_fp32_out != 0 when
 * the handle has been switched to the fp32 matrix instructions.  Synchronises the device. */
int c3_model_range_status(c3_model *m, int *flag_out, int *on_fp32_out);
/* Pileup only: windows gathered on the device out of ONE region matrix instead of `batch` pre-sliced
 * copies.  region_host: (n_cols, C) int8|int32|int64 counts exactly as calculate_clair3_pileup returns them for a region
 * (src/clair3_pileup.h:113; preprocess/CreateTensorPileupFromCffi.py:143-146) -- C3_DTYPE_I64 is plp_data.matrix itself
 * (size_t), narrowed to int32 while it is staged, so the numpy copy of :143-146 is not needed either; starts_host[b] = first column of window
 * b, i.e. the `offset` the reference slices at (CreateTensorPileupFromCffi.py:362-364: result[0][offset:offset+33]).
 * Equivalent to c3_predict on the sliced windows, bit for bit (neither rescales deep windows: c3_predict_pileup_region_depth below does);
 * candidate filtering stays with the caller here (c3_predict_pileup_candidates below takes positions and filters).  Blocks on slot 0 of the ring (c3_predict_submit_region + c3_predict_wait). */
int c3_predict_pileup_region(c3_model *m, const void *region_host, int x_dtype, int64_t n_cols, const int32_t *starts_host,
                             int64_t batch, float *y_host);
/* The region entry on the ring: c3_predict_pileup_region split like c3_predict_submit / c3_predict_wait, on the same slots and lanes
 * (the lane follows `batch`, as for windows); region_host, starts_host and depth_host may be reused as soon as submit returns.
 * depth_host may be NULL (no rescaling) or carry one depth per window (see c3_predict_depth below).  The slot keeps the starts and
 * depths on the device with the region, so the range guard of c3_predict_wait gathers -- and rescales -- again from the original
 * matrix.  The two blocking region entries are this submit + c3_predict_wait on slot 0: same rows as before, now with the guard. */
int c3_predict_submit_region(c3_model *m, const void *region_host, int x_dtype, int64_t n_cols, const int32_t *starts_host, int64_t batch,
                             const int32_t *depth_host, float *y_host, int slot);
/* ---- windows of very deep coverage: the reference's CPU-branch meaning of a pileup window ----
 * Both in-process loops of the reference bring a window of very deep coverage down to max_depth before the network sees it
 * (clair3/CallVariantsFromCffi.py:278-285, the loop of the default pipeline; clair3/utils.py:104-111, the stdin worker's generator):
 *     depth = int(alt_info.split('-', 1)[0])
 *     if depth > 0 and depth > max_depth * 1.5:  X[i] = X[i] / (depth / max_depth)     (int32 array: truncated towards zero)
 * with max_depth = shared/param_p.py:15 (144 on every platform: windows from depth 217 on).  The *_depth entries apply exactly that
 * on the device, for all 33 x C counts of window b with depth_host[b]: two roundings in double (s = depth / max_depth, then x / s),
 * then towards zero -- numpy's statement, not the exact rational x * max_depth / depth (x = 217, depth = 248: 125, not 126).  A window
 * that is not rescaled passes through bit for bit; a batch without any deep window runs what the entry without depths runs.  The
 * reference's GPU branch (int8 tensor files, CallVariantsFromCffiGPU.py) does NOT rescale and stays mirrored as it is: C3_DTYPE_I8 is
 * refused here, because counts above 127 have already wrapped in such files.  Pileup handles only.
 *   c3_model_set_max_depth         param.max_depth_dict[platform]; default 144; <= 0 is an error
 *   c3_predict_depth               c3_predict with depths; x_dtype C3_DTYPE_I32
 *   c3_predict_submit_depth        c3_predict_submit with depths (wait: c3_predict_wait); depth_host may be reused when it returns
 *   c3_predict_pileup_region_depth c3_predict_pileup_region with depths; C3_DTYPE_I32 | C3_DTYPE_I64.  A column belongs to up to 33
 *                                  windows, each rescaled by the factor of its own candidate: the matrix cannot be pre-scaled
 * depth_host == NULL is an error in these three (the entries without depths keep their names and their behaviour).
 * c3_model_describe reports max_depth= and rescaled=<windows rescaled in the last call>. */
int c3_model_set_max_depth(c3_model *m, int max_depth);
int c3_predict_depth(c3_model *m, const void *x_host, int x_dtype, int64_t batch, const int32_t *depth_host, float *y_host);
int c3_predict_submit_depth(c3_model *m, const void *x_host, int x_dtype, int64_t batch, const int32_t *depth_host, float *y_host, int slot);
int c3_predict_pileup_region_depth(c3_model *m, const void *region_host, int x_dtype, int64_t n_cols, const int32_t *starts_host,
                                   int64_t batch, const int32_t *depth_host, float *y_host);
/* ---- candidate POSITIONS instead of window starts: the reference's selection of pileup windows on the device ----
 * Replaces the loop over all_alt_info_list in preprocess/CreateTensorPileupFromCffi.py:343-397 together with
 * __enforce_pileup_chunk_contiguity (:180-236): the caller hands over the region matrix, plp_data.major and the candidates' positions
 * (the first field of each alt-info string, in the caller's order -- after its own bed / known-VCF filters and the len(alt_info) < 4 skip)
 * and gets the rows of the windows the reference would have fed the model, in the reference's order, plus a status per candidate.
 *   region_host  (n_cols, C) C3_DTYPE_I32, or C3_DTYPE_I64 = plp_data.matrix itself (narrowed while it is staged); C3_DTYPE_I8 is refused
 *   major_host   [n_cols] plp_data.major, strictly increasing.  Only `major` is read: the Clair3 pileup emits no minor (insertion) columns
 *   pos_host     [n_cand] candidate positions; depth_host [n_cand] or NULL: with depths, kept windows deeper than 1.5 x max_depth are
 *                rescaled exactly as c3_predict_*_depth does (after selection; zero rows stay zero)
 *   head_tail    != 0: --enable_variant_calling_at_sequence_head_and_tail
 * The rule.  Chunks are the maximal runs of major with steps of exactly 1, first / last a chunk's first and last major; a candidate belongs to
 * the one chunk with first <= pos <= last.  Its window covers positions pos-17 .. pos+15 (the reference's offset = start - first - 1 with
 * start = pos - 16; the asymmetry is the reference's).
 *   main (pos-17 >= first and pos+17 <= last): 33 in-chunk columns; C3_CAND_MAIN unless one of them is all zero over its C counts:
 *        C3_CAND_EMPTY_COLUMN, no row;
 *   with head_tail, where the main test failed:  pos-17 < first: C3_CAND_HEAD iff pos+15 <= last, the columns before first are zero rows;
 *        else (pos+17 > last): C3_CAND_TAIL, the columns after last are zero rows.  These windows are not tested for empty columns;
 *   everything else: C3_CAND_NO_WINDOW, no row.  No candidate yields two windows.
 * Results: status_host[n_cand] (C3_CAND_*), *n_rows_host = number of kept candidates (MAIN, HEAD, TAIL), y_host rows [0, *n_rows_host) in
 * candidate order, c3_model_row_size() floats each (decoder columns apply); y_host must hold n_cand rows.  Rows are bit-identical to c3_predict
 * (c3_predict_depth) on the materialised windows.  The forward pass runs on n_cand windows (the host does not know the count when it
 * submits; a dropped candidate costs one surplus window); n_cand == 0 launches nothing.
 * c3_predict_submit_candidates is completed by c3_predict_wait(slot), which writes rows, statuses and *n_rows_host: same ring, lanes and range
 * guard as c3_predict_submit_region (the slot keeps the selected starts and depths on the device for a re-run on fp32); region, major,
 * positions and depths may be reused as soon as submit returns.  c3_predict_pileup_candidates = submit + wait on slot 0.
 * Errors: a full-alignment handle, C3_DTYPE_I8, major not strictly increasing, null buffers, a busy slot.
 * c3_model_describe reports candidates=, kept=, chunks= of the last completed candidate call. */
#define C3_CAND_NO_WINDOW 0
#define C3_CAND_MAIN 1
#define C3_CAND_EMPTY_COLUMN 2
#define C3_CAND_HEAD 3
#define C3_CAND_TAIL 4
int c3_predict_submit_candidates(c3_model *m, const void *region_host, int x_dtype, int64_t n_cols, const int64_t *major_host,
                                 const int64_t *pos_host, const int32_t *depth_host, int64_t n_cand, int head_tail, float *y_host,
                                 uint8_t *status_host, int64_t *n_rows_host, int slot);
int c3_predict_pileup_candidates(c3_model *m, const void *region_host, int x_dtype, int64_t n_cols, const int64_t *major_host,
                                 const int64_t *pos_host, const int32_t *depth_host, int64_t n_cand, int head_tail, float *y_host,
                                 uint8_t *status_host, int64_t *n_rows_host);
/* ---- full-alignment windows as their OCCUPIED ROWS: the zero rows are restored on the device ----
 * A full-alignment window is depth x positions x C int8, but only the reads that overlap the candidate fill rows.  The reference's stream
 * format carries just those rows and its generator pads them to the matrix depth on the host before the model call (clair3/utils.py:113-121:
 * padding_depth = depth - tensor_depth, prefix = int(padding_depth / 2), the rest behind); its C producer lays the dense matrix out by the same
 * rule (src/clair3_full_alignment_dwell.c:139-150, prefix_padding_depth = padding_depth >> 1).  These entries take the rows and restore the
 * zero rows on the device, bit for bit what c3_predict computes on the padded windows -- and stage, per window, its rows instead of depth rows.
 *   rows_host   the occupied rows of all windows, back to back, positions x C int8 bytes each; window b owns row_count[b] rows starting at
 *               row sum(row_count[0 .. b)).  Full-alignment handles, int8 only
 *   meaning     dense window b is zero except rows [first, first + row_count[b]), which are window b's rows in order.
 *               row_first == NULL: first = (depth - row_count[b]) / 2 (integer division) -- the reference's rule;
 *               row_first != NULL: first = row_first[b], the caller says where the run sits (any dense window can be carried losslessly)
 *   errors      before anything is queued, the slot left free: a pileup handle, null buffers with batch > 0, row_count[b] < 0, first < 0,
 *               first + row_count[b] > depth, a busy slot.  row_count[b] == 0 is a legal all-zero window; batch == 0 launches nothing
 * Same ring, lanes, decoder columns and range guard as c3_predict_submit: the slot keeps the rows and their table on the device, never writes
 * them, and a re-run on fp32 expands again from them.  rows_host, row_first and row_count may be reused as soon as submit returns.
 *   c3_predict_submit_rows   completed by c3_predict_wait(slot)
 *   c3_predict_rows          submit + wait on slot 0
 *   c3_pack_rows             plain host code (no device, like c3_vcf_rows): for each of `batch` dense windows at x_host the run from its first
 *                            to its last non-zero row (interior zero rows stay inside the run; an all-zero window: count 0, first 0) copied
 *                            to rows_out (may be sized for batch x depth rows; NULL: only the counts), row_first_out / row_count_out filled.
 *                            Returns the number of rows, < 0 on error.  Only zero rows and the two boundary rows are read besides the copy.
 * C3HIP_PACK_ROWS=1 (read at c3_model_create; default off): c3_predict / c3_predict_submit of a full-alignment handle pack the int8 windows
 * they are given while they stage them and continue as c3_predict_submit_rows with explicit firsts; rows are bit-identical either way.
 * c3_model_describe of a full-alignment handle ends on rows_windows=<windows that travelled as rows> rows_shipped=<their rows>
 * pack_rows=<0|1> for the last completed call. */
int c3_predict_submit_rows(c3_model *m, const void *rows_host, const int32_t *row_first, const int32_t *row_count, int64_t batch,
                           float *y_host, int slot);
int c3_predict_rows(c3_model *m, const void *rows_host, const int32_t *row_first, const int32_t *row_count, int64_t batch, float *y_host);
int64_t c3_pack_rows(int depth, int positions, int channels, const void *x_host, int64_t batch, void *rows_out, int32_t *row_first_out,
                     int32_t *row_count_out);
/* SURVEY 8f N1 (first slice): the arithmetic of the reference decoder, clair3/CallVariants.py:510-659
 * (possible_outcome_probabilites_from).  For every probability row y_host[b] (24 or 90 floats, as produced by
 * c3_predict) and the gt21 index of its reference base pair ref21_host[b] (0 AA, 4 CC, 7 GG, 9 TT -- reference_gt21 at
 * :520,:570), computes for the ten outcome classes in the order of the reference's max(...) call (:722-733: homo_Ref,
 * homo_SNP, hetero_SNP, homo_Ins, homo_Del, hetero_ACGT_Ins, hetero_InsIns, hetero_ACGT_Del, hetero_DelDel,
 * hetero_InsDel) the maximum of the class's probability list and the position of its first occurrence in the
 * reference's enumeration order, plus early_host[b] = 1 where the reference takes the homo-reference early exit
 * (:532-534, :573-576).  Products are float32 in the reference's multiplication order: the values are bit-identical
 * to the numpy float32 scalars of the reference, so `maximum_probability in <class list>` (:741-749) equals
 * `maxp[b][class] == max over classes`.  Allele strings, alt_info and the retry loop stay in Python.
 * maxp_host: [batch][10] float, argmax_host: [batch][10] int32, early_host: [batch] bytes.  Synchronous. */
int c3_outcome_maxima(c3_model *m, const float *y_host, int64_t batch, const uint8_t *ref21_host, float *maxp_host,
                      int32_t *argmax_host, uint8_t *early_host);
/* The decoder columns for rows that are already on the host: rows_host[batch][output_size + C3_DECODE_COLS] receives
 * y_host[b] followed by its columns (same kernel as the c3_model_set_decode_columns path).  Synchronous. */
int c3_decode_columns(c3_model *m, const float *y_host, int64_t batch, float *rows_host);
/* SURVEY 8f N1, the host side of the decoder: the VCF text of the rows of a batch whose first decision stands, in one pass over the
 * batch -- what clair3/CallVariants.py does per row in batch_output (:1069-1116) -> output_with (:1119-1394) -> output_from's first
 * pass (:676-1008) with the allele lookups find_alt_base (:662-673), insertion_ / deletion_bases_using_alt_info_from (:117-201), for
 * rows that carry the decoder columns.  Plain host code (no device, safe in the forked decode workers of
 * clair3/CallVariantsFromCffi.py:302-353).  An accelerator of clair3_amd/vcf_rows.py, not a second decoder: rows that are not
 * plainly the common case get status 1 and are printed by the caller's Python path (the walk over rejected candidates, shared
 * maxima, odd bytes).
 *   cfg         what the reference's OutputConfig / param say: width 24|90, flank = param.flankingBaseNum, show_reference,
 *               keep_iupac, has_qs_pass / qs_pass = quality_score_for_pass, pileup ('P' / 'F' in INFO), max_len = VariantLength.max,
 *               infer = maximum_variant_length_that_need_infer, phred_trans = CallVariants.Phred_Trans, f32_arith = 1 when the
 *               caller's numpy evaluates `1.0 - float32` in float32 (numpy >= 2: quality_score_from :375-381 depends on it),
 *               gt[4] = genotype_string_from of homo_reference, homo_variant, hetero_variant, hetero_variant_multi; walk = 1: rows
 *               whose first candidate the reads do not offer are walked here too (the later passes of output_from's loop), 0: handed back
 *   pos_text / alt_text   the n chr_pos_seq / alt_info strings, NUL-separated
 *   rows        n rows of row_stride_floats floats: width probabilities + C3_DECODE_COLS columns
 *   out, out_off[n + 1], status[n]   text of row i = out[out_off[i] .. out_off[i + 1]) when status[i] is 0 (first decision) or 2 (after
 *               rejected candidates); empty: the reference prints nothing for it.  status[i] == 1: the caller prints the row itself */
typedef struct {
    int32_t width, flank, show_reference, keep_iupac, has_qs_pass, pileup, max_len, infer, f32_arith, walk;
    int32_t gvcf, haploid;  /* gvcf: rows carry the PL field (output_config.gvcf, clair3/CallVariants.py:1360-1378, compute_PL :1397-1454);
                             * haploid: bit 0 is_haploid_precise_mode_enabled, bit 1 is_haploid_sensitive_mode_enabled (:1191-1199, :1327-1329) */
    int32_t long_indel, long_infer;  /* --enable_long_indel (and not param.cal_precise_long_indel_af): the reads of insertion alleles within long_prop of a
                                      * long allele's length count with it (get_long_indel_read_count, clair3/CallVariants.py:383-402); long_infer =
                                      * param.maximum_variant_length_that_need_infer (50), long_prop = param.long_indel_distance_proportion (0.1) */
    double qs_pass, phred_trans, long_prop;
    char gt[4][8];
} c3_rows_config;
int c3_vcf_rows(const c3_rows_config *cfg, int64_t n, const char *pos_text, int64_t pos_bytes, const char *alt_text, int64_t alt_bytes,
                const float *rows, int64_t row_stride_floats, char *out, int64_t out_cap, int64_t *out_off, uint8_t *status);
/* ---- the collective of the sharded job ----
 * The reference meets its per-GPU workers on disk (one VCF shard per worker, merged by SortVcf:
 * clair3/CallVariantsFromCffiGPU.py:138-199, preprocess/SortVcf.py:290-362).  Here the probability rows of every
 * rank's window shard travel to one rank in a single gather(v), issued DIRECTLY on RCCL (grouped ncclSend / ncclRecv
 * over xGMI, librccl bound with dlopen) on the caller's HIP stream, ordered behind the forward pass on that stream.
 *   c3_comm_unique_id   rank 0 fills 128 bytes (ncclGetUniqueId); the caller hands them to every rank (any control
 *                       plane: a file, the launcher's store) -- rendezvous is not this library's business
 *   c3_comm_create      every rank, same id; world == 1 needs no id and no RCCL (the gather is a device copy) -- unless the
 *                       environment says C3HIP_FORCE_RCCL=1 (test knob): then a world of one makes its own id and a one-rank
 *                       communicator (ncclCommInitRank, nranks = 1) and its gather is a grouped self ncclSend / ncclRecv, so
 *                       the whole call sequence meets the real librccl on a one-GPU box (tests/test_comm_gpu.py)
 *   c3_gather_rows      rows_dev: this rank's counts[rank] rows of row_floats floats (device); counts: rows of every rank
 *                       (host, identical on all ranks -- they follow from the shard ranges); all_dev (rank dst only):
 *                       sum(counts) rows, rank-major = window order for contiguous shards.  Asynchronous on `stream`. */
typedef struct c3_comm c3_comm;
int c3_comm_unique_id(void *id128);
c3_comm *c3_comm_create(const void *id128, int rank, int world, int device);
int c3_comm_destroy(c3_comm *c);
int c3_gather_rows(c3_comm *c, const float *rows_dev, int row_floats, const int64_t *counts, float *all_dev, int dst, void *stream);
/* what RCCL itself says about the communicator (ncclCommCount / ncclCommUserRank): *ranks_out ranks, this one *rank_out
 * (may be NULL); world == 1 answers without RCCL.  bench.py prints it as rccl_ranks_seen. */
int c3_comm_count(c3_comm *c, int *ranks_out, int *rank_out);
/* give up on a collective that does not complete (ncclCommAbort); from then on c3_gather_rows on this handle is the local
 * copy of THIS rank's rows (counts[] stays the caller's array over the original ranks; all_dev is required) and the caller
 * routes its rows another way (clair3_amd/dist.py falls back to torch.distributed) */
int c3_comm_abort(c3_comm *c);
/* watchdog for work queued on `stream` of `device` (hipStreamQuery polled every 50 us): 0 = finished, 1 = still running after
 * timeout_ms (c3_last_error() == "timeout"; timeout_ms < 0 waits for ever), other = error */
int c3_stream_wait(void *stream, int device, int timeout_ms);
/* A hint, not a requirement: how many handles the CALLER keeps feeding this GPU side by side (default 1 -- the worker of
 * clair3/CallVariantsFromCffiGPU.py:163-199 after callvar.install(): one process, one handle per GPU).  Tile shapes of the pileup
 * kernels follow it (alone: 8-window LSTM tiles and 240 projection workgroups so that a 1024-window batch reaches every CU;
 * sharing: 16-window tiles and 120 workgroups, because the other batches fill the rest).  Rows are bit-identical either way. */
int c3_model_set_sharing(c3_model *m, int handles);
/* ---- verify mode: the fp16x3 rows of a job's own batches against the fp32 forms, compared on the device ----
 * The product path stays on the fp16x3 kernels because of four decisions -- the per-channel weight scales, the channel equalisation at
 * load, the 16000 range guard, the load-time |w| >= 4 rule -- that have only ever met synthetic weights ("parity on a
 * TRAINED checkpoint is unpinned").  This is the instrument for a caller who has a real checkpoint: inside the job they run anyway, every
 * `every`-th batch submitted to the submit / wait ring (c3_predict_submit and every entry built on it: the pieces of a blocking c3_predict,
 * depths, regions, candidates, rows) also runs on the fp32-MFMA forms from the same staged input, and the two sets of rows are compared
 * where they are.  The record comes back with the batch and adds up on the handle.
 *   every       0 = off.  The submits of a handle with batch > 0 are numbered from 0 (from the last load / reset on); number k is selected
 *               when k % every == 0.  A selected batch is SKIPPED (counted, not verified) when the handle is already on the fp32 forms,
 *               when c3_debug_keep_activations, c3_debug_tap or c3_profile_enable is on (the second pass must not overwrite what they
 *               record), when a candidate batch has nothing to launch, or when the range guard answered the batch (it keeps priority)
 *   tol         > 0: a row counts in rows_over_tol when any of its probabilities differs by more than tol
 *   near_tie    >= 0: an arg-max difference in a head whose fp32 top-2 gap is at most near_tie is excused (counted in near_ties)
 *   policy      C3_VERIFY_REPORT: the caller gets the fp16x3 rows, bit for bit what a run without verify mode returns.
 *               C3_VERIFY_ESCALATE: a batch with rows_over_tol > 0 or an arg-max difference outside near-ties is answered with its fp32
 *               rows (decoder columns included; c3_predict_submit_dev: they replace the rows on the device), one line goes to stderr and
 *               the handle continues on the fp32 forms (c3_model_describe: precision=fp32-verify).  Batches of other slots that are in
 *               flight on fp16x3 and were not selected keep their rows: they are as unverified as any batch before them
 * Compared per row and head (columns 0-21-24-57-90, the decoder columns are not): |a - b| in fp32, the arg-max, the fp32 row's top-2 gap;
 * for a candidate batch only the rows of kept candidates.  With verify mode never enabled on a handle nothing is allocated or launched.
 * c3_predict_device and c3_predict_device_checked are asynchronous entries on the CALLER's stream: they stay exactly as they are and are
 * never verified.  Refused while a c3_predict_submit of the handle is pending.
 *   c3_model_verify_stats   the totals since the last c3_model_load / c3_model_verify_reset (a reload resets them and keeps the setting)
 *   c3_model_verify_reset   zero the totals (and the numbering of the submits)
 * c3_model_describe ends on verify=... while verify mode is or was on for the handle. */
#define C3_VERIFY_REPORT 0
#define C3_VERIFY_ESCALATE 1
typedef struct {
    int64_t batches_submitted;  /* submits with batch > 0 while verify mode was on */
    int64_t batches_checked;    /* ... compared */
    int64_t batches_skipped;    /* ... selected but not compared (see above) */
    int64_t windows_checked;    /* rows compared */
    int64_t worst_batch;        /* number of the submit with the largest |d| (-1: none checked yet) ... */
    int64_t worst_row;          /* ... and the lowest row inside it that reaches it */
    int64_t rows_over_tol;
    int64_t label_diffs[4];     /* per head: arg-max differences outside near-ties */
    int64_t near_ties[4];       /* per head: arg-max differences excused as near-ties */
    int64_t escalations;
    float max_abs_diff;
    float head_max_abs_diff[4];
    float tol, near_tie;        /* the setting in force */
    int32_t every, policy;
} c3_verify_stats;
int c3_model_set_verify(c3_model *m, int every, float tol, float near_tie, int policy);
int c3_model_verify_stats(c3_model *m, c3_verify_stats *out);
int c3_model_verify_reset(c3_model *m);
/* ---- layer records of verify mode: WHERE the two forms differ ----
 * With c3_model_set_verify_layers(m, 1) every batch that verify mode selects and compares also compares, per layer, the output a of the
 * product (fp16x3) form with the output b of the fp32 form -- both from the same staged input, both in the checkpoint's units (the values
 * c3_debug_tap_fetch returns), on the device, for all windows of the batch (a candidate batch: the kept ones).  The product pass keeps its
 * layer outputs with the tap mechanism's copies into buffers of the slot, so the kernel forms, c3_model_describe and the rows stay what
 * they are; a batch that verify mode skips brings no layer record.  It has no effect while every == 0; with it never enabled nothing is
 * allocated or launched and verify mode is what it is without it.  Refused while a c3_predict_submit of the handle is pending.
 * Layers, in network order, under the tap names: full alignment act0 .. act8, spp, l4_out; pileup lstm1_out, gx2, lstm2_out, l4_out.  A
 * layer the product form does not materialise (default forms: act0 inside res1a, act8 inside res3b) is not compared: status FUSED.
 *   c3_model_verify_layers   fills up to max_entries entries and returns the number of layers (0: never enabled on this handle; < 0: error).
 *                            Totals since the last c3_model_load / c3_model_verify_reset (both zero them and keep the setting)
 * Per layer: |a - b| in fp32 (a value that is not finite counts as +inf); worst_*: the first batch that reached a strictly larger
 * max_abs_diff, the lowest (window, index) in it that reaches it -- index: the flat index inside the window in the order of
 * c3_debug_tap_fetch (NHWC for act*, (bin, c) for spp, (t, feature) for the pileup tensors).
 * c3_model_describe appends ,layers:1 to its verify=... text while the switch is on. */
#define C3_VERIFY_LAYER_NONE 0     /* no batch with layer records yet */
#define C3_VERIFY_LAYER_COMPARED 1
#define C3_VERIFY_LAYER_FUSED 2    /* the product form computes it inside a fused kernel: not compared */
typedef struct {
    char name[16];
    int32_t status;         /* C3_VERIFY_LAYER_* */
    int32_t reserved;
    int64_t batches;        /* batches in which the layer was compared */
    int64_t windows;        /* ... and their windows */
    int64_t worst_batch;    /* number of the submit (as c3_verify_stats.worst_batch; -1: none yet) ... */
    int64_t worst_window;   /* ... the window inside it ... */
    int64_t worst_index;    /* ... and the flat index inside that window */
    float max_abs_diff;     /* max |a - b| */
    float ref_max_abs;      /* max |b| */
    float test_max_abs;     /* max |a| */
    float reserved2;
} c3_verify_layer;
int c3_model_set_verify_layers(c3_model *m, int enable);
int c3_model_verify_layers(c3_model *m, c3_verify_layer *out, int max_entries);
/* which kernel forms the handle's last forward pass took, as "key=value ..." text; bench.py reports it next to its rates */
/* ---- per-layer precision: named layers on their fp32-MFMA forms, the rest of the handle on fp16x3 ----
 * Precision used to be a property of the whole handle: C3HIP_FP32=1, the range guard and the load-time rule move EVERY layer off the 16-bit
 * matrix instructions.  A plan names the layers that run their fp32 form; every other layer keeps its product kernel, and activations
 * cross the boundary in the layout the neighbour reads (plane activations stay planes: c3_gemm.h ConvPlanesLoader, c3_lstm_fused.h).
 *   names       comma separated layer names, "" = none (the default), "all" = every layer (the handle then runs exactly what C3HIP_FP32=1 runs).
 *               pileup: lstm1, proj2, lstm2, l4        full alignment: conv1, res1a, res1b, conv3, res2a, res2b, conv5, res3a, res3b, l4
 *               (the FC tail is fp32 in both forms and has no name; naming a layer twice is accepted)
 * An unknown name, a name of the other network and an empty entry between commas are errors that name the entry and leave the plan as it
 * was; so is a call while a c3_predict_submit of the handle is pending.  The plan belongs to the handle: it survives c3_model_load and
 * applies to every entry and lane, the device-resident ones included.  A full-alignment plan that names conv1, res1a or res1b runs conv1 as
 * its own launch (as C3HIP_CONV1_FUSED=0), one that names res3b the pooling (as C3HIP_SPP_FUSED=0).  The range guard is unchanged (a raised
 * flag moves the whole handle to fp32 for good); verify mode compares the plan's rows and layer outputs with the all-fp32 forms.
 * env C3HIP_FP32_LAYERS=<names>: the plan a handle starts with (an invalid value makes c3_model_create fail with that message);
 * env C3HIP_AUTO_FP32_LAYERS=<names>: what the load-time rule escalates INSTEAD of the whole handle (c3_model_describe:
 * precision=fp32-auto(<names>), on_fp32=0).  C3HIP_FP32=1 wins over both; with C3HIP_FP32=0 an explicit plan still applies.
 *   c3_model_layer_precision   the plan in force, network order ("" = none)
 *   c3_layer_precision_check   plain host code, no device: 0, or != 0 with c3_last_error() naming the bad entry
 * c3_model_describe gains fp32_layers=<names> only while a plan is in force. */
int c3_model_set_layer_precision(c3_model *m, const char *names);
int c3_model_layer_precision(c3_model *m, char *buf, int buf_bytes);
int c3_layer_precision_check(int kind, const char *names);
/* ---- full alignment: channel exponents calibrated from observed activations (DESIGN.md 1 Range) ----
 * The reference keeps its activations in fp32 (clair3/model.py:377-416, torch conv2d + BatchNorm2d in eval mode) and has no range to mind.
 * Here they live as fp16 piece pairs: c3_model_load gives every channel an exact power of two 2^k0 from its BatchNorm's gamma and beta, and
 * the range guard (see c3_predict) moves a handle whose activations reach 16000 all the same to the fp32 matrix instructions for good.
 * Calibration measures instead: a sample of the job's own windows runs on the fp32 forms, a census takes max |x| of every convolution's
 * output channels, and a rule turns it into a LOWERING per channel -- by how many powers of two its exponent comes down, k = k0 - lowering.
 * Exact rescaling, as at load time: the rows are those of the checkpoint as given.  Opt-in; a handle without a lowering packs and runs what
 * it did before these entries existed.
 *   channels    896 = 2 x (64 + 128 + 256), the groups in the order stage0, inner0, stage1, inner1, stage2, inner2: stage s = the outputs
 *               of convolutions 3 s and 3 s + 2 (one exponent for both: the residual add), inner s = the output of convolution 3 s + 1
 *   c3_model_calibrate             runs the windows on the fp32 forms in the handle's first lane, blocking, and adds them to the census;
 *                                  y_host (may be NULL) receives their rows, [batch][c3_model_row_size].  It leaves the handle's precision, range
 *                                  flag, verify totals and what c3_model_describe reports of the last predict call as they are
 *   c3_model_calibrate_reset       zeroes the census and its window count (the census outlives c3_model_load: reset it with a new checkpoint)
 *   c3_model_calibration_census    absmax_out[9][256]: max |x| per convolution and channel in the CHECKPOINT's units (the same whatever
 *                                  exponents the handle ran with), entries beyond a layer's channels 0; windows_out: windows counted.  Either may be NULL
 *   c3_model_calibration_solve     the rule on the census and the k0 of the last load, group by group: for a stage the larger of its two layers
 *   c3_calibration_rule            the rule for ONE group of n channels, plain host code, no device: with s[c] = scaled_max[c] = f * 2^e, f in
 *                                  [0.5, 1): d[c] = max(0, e - cap_log2) (0 for s[c] = 0); d_group = the lower median of d over the channels
 *                                  with s[c] > 0 (0 without one); lowering[c] = max(d[c], d_group) for EVERY channel -- a channel the sample
 *                                  left silent follows its group.  cap_log2 in [4, 13]; 10 leaves 16000 / 2^10 = 15.6 x for windows the sample
 *                                  did not contain and is 50 x above what ordinary checkpoints reach.  A value that is not finite is an error
 *                                  that names the channel (c3_model_calibration_solve: the layer and the channel).  The solve additionally keeps
 *                                  k0 - lowering >= -40, the clamp of the load-time rule
 *   c3_model_set_channel_lowering  lowering[896], NULL = none.  Takes effect at the next c3_model_load; belongs to the handle like the precision
 *                                  plan: it survives loads and applies to every entry and lane
 *   c3_model_channel_exps          k0_out[896] / k_out[896] of the last load (either may be NULL): k0 identifies the checkpoint a lowering was made for
 * All but c3_calibration_rule: full-alignment handles only (the gates of the pileup network's LSTMs are not homogeneous) and refused while a
 * c3_predict_submit of the handle is pending.  The range guard, verify mode (which compares the calibrated product rows with the fp32 forms on
 * the same packed weights) and the precision plan are unchanged.  c3_model_describe gains calibration=cap:<n>,windows:<n>,lowered:<channels>
 * only while a lowering is set.  cap and windows describe the lowering in force and are recorded with it: c3_model_set_channel_lowering takes
 * them from the handle's last solve where the lowering is that solve's result, else 0 (not known), and
 *   c3_model_set_calibration_origin   states them for a lowering made elsewhere (cap_log2 in [0, 13], windows >= 0; what a calibration file carries).
 * What the census pass does leave behind: the first lane's workspace holds ITS activations, so c3_debug_fetch after c3_model_calibrate returns
 * those (fp32 forms) and not the last predict call's; tap buffers (c3_debug_tap) and a profile being taken (c3_profile_enable) are not touched. */
int c3_model_calibrate(c3_model *m, const void *x_host, int x_dtype, int64_t batch, float *y_host);
int c3_model_calibrate_reset(c3_model *m);
int c3_model_calibration_census(c3_model *m, float *absmax_out, int64_t *windows_out);
int c3_model_calibration_solve(c3_model *m, int cap_log2, uint8_t *lowering_out);
int c3_model_set_channel_lowering(c3_model *m, const uint8_t *lowering);
int c3_model_set_calibration_origin(c3_model *m, int cap_log2, int64_t windows);
int c3_model_channel_exps(c3_model *m, int8_t *k0_out, int8_t *k_out);
int c3_calibration_rule(const float *scaled_max, int n, int cap_log2, uint8_t *lowering_out);
/* ---- the range-guard policy: recalibrate on a trip and stay on the fp16x3 kernels (full alignment; DESIGN.md 1 Range) ----
 * The range guard (see c3_predict) answers a trip by running the batch again on the fp32 forms -- and, by default, leaves the handle there
 * for the rest of its life.  That re-run is an fp32 pass over exactly the windows that tripped: under C3_RANGE_RECALIBRATE the guard takes
 * the census of c3_model_calibrate during it, solves (c3_model_calibration_solve at the cap of the lowering in force, else 10; the new
 * lowering is the element-wise maximum of the old and the solved one: never up), packs the weights again from a private host copy of the
 * float32 tensors of the last load and continues on the fp16x3 kernels.  The rows that answer the batch are those of the fp32 re-run, bit
 * for bit what the sticky guard returns.  Opt-in: with no policy set nothing changes.
 *   c3_model_set_range_policy   policy C3_RANGE_STICKY (the default) or C3_RANGE_RECALIBRATE; max_recalibrations >= 0 bounds how often the
 *                               handle may recalibrate between two loads (0 behaves as sticky).  Refused while a c3_predict_submit is
 *                               pending; RECALIBRATE is refused on a pileup handle (LSTM layers have no ReLU homogeneity to rescale
 *                               through) and on a loaded handle that holds no copy of its tensors: set it before c3_model_load.  While the
 *                               policy is RECALIBRATE c3_model_load keeps that copy (about 12 MB for this network), freed with the handle
 *                               or when the policy goes back to sticky
 *   c3_range_policy_check       plain host code, no device: 0 for "sticky", "recalibrate" and "recalibrate:<n>" (n = max_recalibrations,
 *                               default 4), else != 0 with c3_last_error() saying what is expected
 *   c3_model_range_stats        the totals since the last c3_model_load
 * Where it applies: c3_predict_wait -- and so the blocking c3_predict* entries -- and c3_predict_device_checked; c3_predict_device is
 * unchanged.  Before the weights are packed again the guard waits for the device work of every other batch in flight; such a batch, should
 * its own flag copy be raised (the flag word is sticky) or a row of it not be finite, runs again on the fp16x3 kernels with the new weights
 * when its c3_predict_wait comes and is then checked like a fresh batch.  The handle falls back to the sticky behaviour for this and all
 * later batches when the solve lowers nothing further, when the census is not finite or when the allowance is used up; stderr then carries
 * the sticky guard's sentence and the reason.  A repack does not touch the precision plan, verify mode's totals, taps, a profile or the
 * exact form's weights.  Verify mode: the guard keeps priority.  A lowering set before (c3_model_set_channel_lowering, a calibration file)
 * is where the handle starts from.  After a recalibration the lowering in force is k0 - k of c3_model_channel_exps, its origin cap_log2 and
 * census_windows below.
 * env C3HIP_RANGE_GUARD=<text of c3_range_policy_check>: the policy a full-alignment handle starts with (an invalid value makes
 * c3_model_create fail with that message; a pileup handle ignores it).
 * c3_model_describe gains range_guard=recalibrate,recalibrations:<n>[,fell_back] only while a policy other than sticky is set. */
#define C3_RANGE_STICKY 0
#define C3_RANGE_RECALIBRATE 1
typedef struct {
    int64_t trips;             /* batches that came back out of range while the policy was RECALIBRATE */
    int64_t recalibrations;    /* ... answered by packing the weights again */
    int64_t reruns;            /* batches in flight across a recalibration that ran again on the new weights */
    int64_t census_windows;    /* windows in the handle's census (c3_model_calibration_census) */
    int32_t channels_lowered;  /* channels whose exponent the last recalibration moved */
    int32_t cap_log2;          /* the cap of the last recalibration's solve */
    int32_t policy, max_recalibrations;  /* the setting in force */
    int32_t fell_back;         /* != 0: the handle went back to the sticky behaviour ... */
    char reason[96];           /* ... and why ("" otherwise) */
} c3_range_stats;
int c3_model_set_range_policy(c3_model *m, int policy, int max_recalibrations);
int c3_range_policy_check(const char *text);
int c3_model_range_stats(c3_model *m, c3_range_stats *out);

/* ---- the exact form: both networks in fp64 from end to end on the device (csrc/c3_exact.h) ----
 * The arithmetic of oracle/c3_oracle.c at the speed of the chip: the checkpoint's fp32 weights widened to double, every product, sum,
 * activation and intermediate tensor double (v_mfma_f64_16x16x4_f64; exp, tanh, expm1 the double-precision library functions);
 * BatchNorm with eps 1e-3 and running statistics (clair3/model.py:191,195-197), folded in double; the full-alignment input x / 100
 * (model.py:378); LSTM gate order i, f, g, o with both biases (model.py:132-133); SELU before the soft-max (model.py:142-150).  No channel
 * exponent, no weight scale, no calibration lowering: the precision plan and the handle's fp32 / range-guard state do not enter.
 * An instrument for measuring the other forms against the exact row (python -m clair3_amd.audit), not a path of a pipeline.
 *   c3_model_set_exact   takes effect at the next c3_model_load (like c3_model_set_channel_lowering): that load also places the double
 *                        weights on the device.  Refused while a c3_predict_submit is pending.  While it was never enabled nothing is
 *                        allocated, uploaded or launched and c3_model_describe is unchanged; while enabled describe ends on " exact=1"
 *   c3_predict_exact     blocking; y_host[batch][c3_model_output_size()] doubles, no decoder columns.  Windows only (x_dtype: pileup
 *                        C3_DTYPE_I8 | C3_DTYPE_I32, full alignment C3_DTYPE_I8, in the geometry of c3_model_set_geometry): regions,
 *                        candidates, depths and rows are materialised by the caller.  The call is cut into passes of at most
 *                        C3HIP_EXACT_CHUNK windows (default 256 full alignment, 1024 pileup) in a workspace of its own (2.2 MB per
 *                        full-alignment window, 0.8 MB per pileup window); a window's row is bit-identical whatever batch or pass it
 *                        travels in.  It runs on the first lane's stream with the device synchronised before and behind, and leaves what
 *                        c3_model_calibrate leaves: precision, range flag, verify totals, taps, a profile being taken and what
 *                        c3_model_describe reports of the last predict call.  batch == 0 launches nothing.  Errors (exact not enabled at
 *                        the last load, a pending submit, a dtype the kind does not take, null buffers) leave the handle usable
 *   c3_exact_fetch       windows [first, first + windows) of the LAST PASS of the last c3_predict_exact call; names and layouts those of
 *                        c3_debug_tap_fetch (full-aln "act0".."act8", "spp", "l4_out"; pileup "lstm1_out", "gx2", "lstm2_out", "l4_out").
 *                        Every tensor exists: nothing is fused here */
int c3_model_set_exact(c3_model *m, int enable);
int c3_predict_exact(c3_model *m, const void *x_host, int x_dtype, int64_t batch, double *y_host);
int c3_exact_fetch(c3_model *m, const char *name, int64_t first, int64_t windows, double *host_out, int64_t n_doubles);

/* ---- the exact form on the submit / wait ring: what answers a batch, what verify mode compares with (csrc/c3_exact.h) ----
 * The exact pass reads a batch of the ring where the product forms read it -- the staged windows; windows with depths and the windows of a
 * region or candidate batch as the pre-pass of c3_rescale.h writes them into the lane's buffer (without a deep window it is a plain gather);
 * occupied rows as c3_expand.h expands them; parts as the one batch they are -- on the batch's lane stream, cut into passes of
 * C3HIP_EXACT_CHUNK windows in the handle's ONE exact workspace (passes of different lanes are put in order by an event).  A small kernel
 * rounds the fp64 rows to float32 (round to nearest even) into the slot's row buffer; decoder columns, score mode and the rows' way back
 * (parts, c3_predict_submit_dev) are what they are for product rows.  A window's float32 exact row is bit-identical whatever batch, chunk,
 * lane or input kind it travelled in: it is (float)c3_predict_exact of that window.  A candidate batch computes a row for every candidate
 * slot, as the product forms do; rows [0, kept) are the result.  An int8 REGION matrix is refused (the gather is the int32 pre-pass).
 *   c3_model_set_answer   C3_ANSWER_EXACT: every batch of the ring -- c3_predict, c3_predict_submit and everything built on it: depths,
 *                         regions, candidates, rows, parts, c3_predict_submit_dev, score mode -- is answered by the float32 rounding of its
 *                         exact rows, decoder columns computed from those rows.  No product or fp32 kernel is launched for such a batch, the
 *                         range flag is neither raised nor read, verify mode skips it (counted in batches_skipped, like a batch of a handle
 *                         on the fp32 forms).  c3_model_describe reports precision=exact; set back to C3_ANSWER_PRODUCT it reports what it
 *                         reported before and the rows are bit for bit those of a handle that never had it set.  Refused unless the last
 *                         c3_model_load placed the double weights (c3_model_set_exact), and while a c3_predict_submit is pending; it
 *                         survives a reload that keeps the exact form, and c3_model_set_exact(m, 0) is refused while it is set.
 *                         c3_predict_device and c3_predict_device_checked stay exactly what they are: the product forms on the caller's stream
 *   c3_model_set_verify_reference   C3_VERIFY_REF_EXACT: a batch verify mode selects runs the exact pass in place of the fp32 pass, and the
 *                         rows are compared with the fp64 rows: |(double)a - b| in double, the arg-max and the top-2 gap of the EXACT row,
 *                         tol and near_tie compared as doubles; the float fields of c3_verify_stats are the round-to-nearest floats of the
 *                         double maxima, the double maximum itself is c3_verify_extra.max_abs_diff_f64.  Skip rules, numbering, totals and
 *                         reset are unchanged (a selected int8 region batch counts as skipped).  C3_VERIFY_ESCALATE answers the tripping
 *                         batch with its float32 exact rows and continues on the fp32 forms as before.  Refused without the double
 *                         weights and while a submit is pending.  With c3_model_set_verify_layers a compared batch compares the product
 *                         layers with the EXACT layers (the tensors c3_exact_fetch names; every one exists, the pileup gx2 included),
 *                         pass by pass behind the exact pass that wrote them: |(double)a - b| in double, the record's floats the roundings
 *                         of the double maxima; FUSED stays what it is for the product side.  c3_model_describe ends its verify=... text
 *                         on ,ref:exact while the reference is exact
 *   C3_VERIFY_REPLACE     third policy of c3_model_set_verify, with either reference: behind the comparison a small kernel overwrites every
 *                         row that is over tol, or has an arg-max difference outside near-ties in any head, with the reference's row (the
 *                         fp32-form row, or the float32 rounding of the exact row); every other row stays bit for bit the product row, the
 *                         handle stays on the forms it was on.  Decoder columns are recomputed for the batch from the rows as they then
 *                         are (the columns of untouched rows do not change).  It works on the device in front of the rows' copy-out, so
 *                         rows left on the device (c3_predict_submit_dev), parts and score mode see the repaired rows.  A candidate batch:
 *                         rows [0, kept) only
 *   c3_model_verify_extra the totals c3_verify_stats has no room for (that struct keeps its size), since the last load / reset */
#define C3_ANSWER_PRODUCT 0
#define C3_ANSWER_EXACT 1
int c3_model_set_answer(c3_model *m, int form);
#define C3_VERIFY_REF_FP32 0
#define C3_VERIFY_REF_EXACT 1
int c3_model_set_verify_reference(c3_model *m, int ref);
#define C3_VERIFY_REPLACE 2 /* third value of c3_model_set_verify's policy */
typedef struct {
    int32_t reference, reserved;        /* C3_VERIFY_REF_* in force */
    int64_t rows_replaced;              /* C3_VERIFY_REPLACE: rows overwritten with the reference's ... */
    int64_t batches_with_replacements;  /* ... in this many batches */
    double max_abs_diff_f64;            /* C3_VERIFY_REF_EXACT: the largest |(double)a - b| of the compared rows (0 under REF_FP32) */
} c3_verify_extra;
int c3_model_verify_extra(c3_model *m, c3_verify_extra *out);
int c3_model_describe(c3_model *m, char *buf, int buf_bytes);
/* blocks until everything enqueued on the model's own stream has finished */
int c3_model_synchronize(c3_model *m);
int c3_model_destroy(c3_model *m);

/* ---- introspection used by the parity tests and bench.py (not needed by a pipeline) ---- */

/* Copy an intermediate activation of the most recent predict call (its last micro-batch) to the host.
 * names: pileup  "lstm1_out" (B,33,256) "lstm2_out" (B,33,320) "l4_out" (B,128)
 *        full-aln "act0".."act8" NHWC conv outputs, "spp" (B,3584), "l4_out" (B,256).
 * n_floats must equal the tensor's element count for the last batch. */
int c3_debug_fetch(c3_model *m, const char *name, float *host_out, int64_t n_floats);
/* enable=1: every layer writes to its own buffer (otherwise three buffers are recycled and only the
 * non-recycled tensors can be fetched).  Also enabled by the environment variable C3HIP_KEEP_ACTIVATIONS. */
int c3_debug_keep_activations(c3_model *m, int enable);

/* Taps: layer outputs of the kernel forms a call really runs (keep mode switches the fused forms off; taps do not).
 * names: comma separated, "" = none.  full-aln "act0".."act8", "spp", "l4_out"; pileup "lstm1_out", "gx2" (B,33,1280: both directions'
 * x-projections of LSTM2 with both biases, PyTorch gate order), "lstm2_out", "l4_out".  Every later call copies each tapped tensor
 * behind the launch that produced it, on that launch's stream, for ALL its windows (micro-batches, ring lanes); with no
 * tap set a call launches exactly what it did before.  Calls on the handle must not overlap while taps are read. */
int c3_debug_tap(c3_model *m, const char *names);
/* windows [first, first + windows) of tapped tensor `name` of the last call, as the checkpoint's fp32 values.  Fails, naming the
 * fusing kernel, when the call's form produced no such tensor (act0 inside res1a, act8 inside res3b). */
int c3_debug_tap_fetch(c3_model *m, const char *name, int64_t first, int64_t windows, float *host_out, int64_t n_floats);

/* ---- score mode: focal loss and arg-max accuracy of labelled windows, evaluated on the device ----
 * The reference's validation pass (clair3/Train.py:87-107 FocalLoss.forward, :210-257 _run_epoch with train=False) on the rows of a batch
 * where they are.  Labels: (batch, c3_model_output_size()) in the row's own column layout [21|3|33|33], C3_DTYPE_I8 or C3_DTYPE_F32 (soft
 * labels work).  Per window and task t: L_t = sum_c w_c * y_c * (-ln q_c) * (1 - q_c)^gamma * y_c with q = min(max(p, 1e-9f), 1.0f) --
 * evaluated in double from the float32 probabilities, the window's value rounded once to float32, the unrounded values summed in a
 * fixed order: the record of a batch is bit-identical across slots, lanes and runs.
 *   c3_model_set_score  enable != 0: gamma >= 0 and class_weights (c3_model_output_size() floats in the row's column layout, or NULL = none)
 *                       apply to every later score entry; enable == 0: off.  Never enabled: nothing is allocated or launched and
 *                       c3_model_describe is what it was; enabled, it gains " score=gamma:<g>,weights:<0|1>".  Refused while a submit is pending.
 *   c3_score_submit     c3_predict_submit of sliced windows plus their labels; y_host may be NULL (the rows then do not cross PCIe: only the
 *                       record, and the windows' values if asked for, do), loss_host ([batch][tasks] floats) may be NULL.  The buffers
 *                       x_host and labels_host may be reused when it returns.  Same ring, lanes and range guard as every batch: a batch the
 *                       range guard re-runs (either policy) or verify mode escalates is scored again on the rows it is answered with.
 *   c3_score_wait       completes it: c3_predict_wait plus the batch's record.  (c3_predict_wait alone also completes a scored batch.)
 *   c3_score            blocking; a batch of two chunks (C3HIP_PREDICT_CHUNK) or more travels as chunks whose records are added in chunk order
 *   c3_score_rows       scores given probability rows (row_floats >= c3_model_output_size() floats each; the first columns count) without a
 *                       forward pass: the reference's rows, the exact form's, adversarial ones
 * A window with a non-finite probability is not hidden: its values are reported as they come out (a NaN passes the clamp) and `nonfinite`
 * counts it.  arg-max: the first maximum, the lowest index on ties, a NaN never.
 * Errors: a handle without c3_model_set_score, a label dtype other than int8 / float32, gamma < 0 or not finite, a class weight that is not finite. */
typedef struct {
    int64_t windows;
    int32_t tasks;       /* 2, or 4 with the indel-length heads */
    int32_t reserved;
    double loss_sum[4];  /* per task: sum over the windows of L_t (the batch mean is loss_sum[t] / windows) */
    int64_t correct[4];  /* per task: windows whose arg-max of p equals the arg-max of y */
    int64_t nonfinite;   /* windows with a probability that is not finite */
} c3_score_result;
int c3_model_set_score(c3_model *m, int enable, float gamma, const float *class_weights);
int c3_score_submit(c3_model *m, const void *x_host, int x_dtype, int64_t batch, const void *labels_host, int label_dtype, float *y_host,
                    float *loss_host, int slot);
int c3_score_wait(c3_model *m, int slot, c3_score_result *out);
int c3_score(c3_model *m, const void *x_host, int x_dtype, int64_t batch, const void *labels_host, int label_dtype, float *y_host, float *loss_host,
             c3_score_result *out);
int c3_score_rows(c3_model *m, const float *rows_host, int row_floats, int64_t batch, const void *labels_host, int label_dtype, c3_score_result *out,
                  float *loss_host);

/* ---- score mode's census: per-class confusion, reliability and near-tie tables of the scored windows, counted on the device ----
 * Replaces asking for every row (rows of 96 - 360 B per window across PCIe) and counting on the host; the reference has nothing of the
 * kind (clair3/Train.py:210-257 returns a loss).  The rule, with its bins, thresholds and fixed-point unit: clair3_amd/csrc/c3_census.h;
 * in numpy: synthetic.score_census.  Per window and task t (K_t = 21, 3, 33, 33 classes), from the float32 probabilities as they come out:
 *   confusion     [truth][pred] += 1 with the arg-maxima the `correct` count of c3_score_result compares: sum == windows, trace == correct[t]
 *   rel_*         conf = p[pred]; finite and in [0, 1]: bin b = min(19, (int)(conf * 20.0f)), rel_windows[t][b] += 1, rel_correct[t][b] +=
 *                 (pred == truth), rel_conf_q32[t][b] += (int64)rint(conf * 2^32) (mean confidence of a bin: rel_conf_q32 / 2^32 /
 *                 rel_windows); otherwise rel_skipped[t] += 1
 *   gap_below     gap = conf - (the best probability among the other classes), float32; [t][k] += (gap < 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1),
 *                 cumulative; a NaN or infinite gap is counted nowhere
 * Integers throughout: the totals do not depend on chunking, slots, lanes or the order of anything.
 *   c3_model_set_score_census  enable != 0: every later scored batch (c3_score_submit / _wait, c3_score, c3_score_rows) fills a table on
 *                       the device behind its record, from the rows it is answered with (a batch the range guard re-runs or verify mode
 *                       escalates or repairs is counted once, on those rows), and whichever of c3_score_wait / c3_predict_wait completes
 *                       it adds the table to the handle's totals.  Needs c3_model_set_score; refused while a submit is pending.
 *                       c3_model_describe's score field then ends on ",census:1".  Off (the default): no section in a staged batch, no
 *                       launch, no byte copied -- a scored batch is what it was.  On: one memset and one launch per batch and 12032 bytes more
 *                       on the batch's way back.
 *   c3_score_census_read   the totals since the last reset (a 24-column model has two tasks: the tables of the other two stay zero)
 *   c3_score_census_reset  zeroes them
 * Errors: a null handle, a null `out`, a handle without score mode, read or reset on a handle that never enabled the census. */
typedef struct {
    int64_t windows;
    int32_t tasks, reserved;
    int64_t confusion[2628];      /* task t from offset 0, 441, 450, 1539: [truth][pred], K_t x K_t */
    int64_t rel_windows[4][20], rel_correct[4][20], rel_conf_q32[4][20];
    int64_t rel_skipped[4];
    int64_t gap_below[4][6];
} c3_score_census;
int c3_model_set_score_census(c3_model *m, int enable);
int c3_score_census_read(c3_model *m, c3_score_census *out);
int c3_score_census_reset(c3_model *m);

/* ---- refine mode: the windows of a batch that sit near a tie are answered by the exact form ----
 * Labels of the product forms and of the fp64 oracle agree outside near-ties; at a near-tie the label depends on which form computed the
 * row.  With refine mode on, the product pass answers a batch as it does without it, two launches behind it measure per window how close
 * the row is to a tie, and c3_predict_wait runs ONLY the windows within `gap` of one through the exact form (c3_predict_exact's arithmetic)
 * and replaces their rows -- probabilities and decoder columns -- by the float32 rounding of the exact ones.  Every other row stays the
 * product row, bit for bit.  With `gap` far above the forms' row error (1e-6 .. 8.5e-6 in the suite; the default of the Python layer is
 * 1e-4) every arg-max of a returned row is the arg-max of the exact row.
 * The rule (clair3_amd/csrc/c3_refine.h; in numpy: synthetic.refine_gaps / refine_select), all in float32:
 *   head gap     per head (21 | 3 | 33 | 33 columns): the largest minus the second-largest value, 0 when the maximum occurs twice
 *   decoder gap  only with decoder columns on: for every reference base A, C, G, T that does not take the early exit (bit b of decoder
 *                column 22) the same gap among the ten class maxima -- decoder column 9 + b and columns 0 .. 8 --, the minimum over those bases
 *   selected     iff any of these gaps is <= gap.  A NaN gap selects nothing: a non-finite row is the range guard's business
 * Stated limit: near-ties inside one outcome class list are caught only through the head gaps they are products of.
 *   c3_model_set_refine  enable != 0: every later batch of sliced windows without depths (c3_predict and its chunks, c3_predict_submit,
 *                       c3_predict_submit_parts, c3_predict_submit_dev) is refined; gap must be finite and >= 0.  Needs the exact form
 *                       loaded (c3_model_set_exact, then c3_model_load) and verify mode off -- the two own the same rows, and
 *                       c3_model_set_verify(every > 0) is refused while refine mode is on.  Refused while a submit is pending.  A load keeps
 *                       the setting and starts the totals again.  Batches that are NOT refined and count in batches_skipped: one the range guard
 *                       answered, a scored batch, a batch of an exact-answer handle, a batch with depths, a region, candidate, rows or
 *                       packed-rows batch, a batch of more than 2^22 windows.  Off (the default): no section in a staged batch, nothing
 *                       allocated, launched or copied.  On: two launches per batch and 256 + 4 * batch bytes more on its way back; a batch
 *                       with selected windows adds the exact passes over them to its c3_predict_wait.
 *                       c3_model_describe gains " refine=gap:<g>,windows:<n>,selected:<n>,changed:<n>" only while the mode is on.
 *   c3_model_refine_stats   the totals since the last load / reset
 *   c3_model_refine_reset   zeroes them
 *   c3_refine_select    the selection alone on rows the caller brings (row_floats == c3_model_output_size(), or that + C3_DECODE_COLS with the
 *                       decoder columns filled in): index_out (batch entries of room) receives the selected windows in ascending order, *n_out
 *                       their number, gaps_out (batch floats, may be NULL) every window's minimum gap (NaN gaps left out; NaN when all are).
 *                       Needs neither the mode nor the exact form.
 * Errors: a null handle or argument, a gap that is negative or not finite, refine with verify mode on, refine without the exact form. */
typedef struct {
    int64_t batches;            /* completed batches of windows while the mode was on = refined + skipped + those with nothing selected */
    int64_t batches_refined;    /* ... with at least one window answered by the exact form */
    int64_t batches_skipped;
    int64_t windows;            /* windows of the batches that were not skipped */
    int64_t windows_selected;   /* ... answered by the exact form */
    int64_t windows_changed;    /* ... in which the arg-max of a head changed between the product row and the exact float32 row */
    int64_t head_selected[4];   /* windows with g_h <= gap, per head */
    int64_t decoder_selected;   /* windows with the decoder gap <= gap */
    float min_gap[4];           /* per head: the smallest gap seen (+inf: none) */
    float max_abs_diff;         /* max |exact float32 - product| over the refined probabilities */
    float gap;                  /* the setting (0 when the mode was never on) */
} c3_refine_stats;
int c3_model_set_refine(c3_model *m, int enable, float gap);
int c3_model_refine_stats(c3_model *m, c3_refine_stats *out);
int c3_model_refine_reset(c3_model *m);
int c3_refine_select(c3_model *m, const float *rows_host, int row_floats, int64_t batch, float gap, int32_t *index_out, int64_t *n_out,
                     float *gaps_out);

/* ---- jackknife mode: the leave-one-read-out stability of full-alignment calls ("Jackknife mode") ----
 * Verify, score and refine mode measure what the ARITHMETIC can do to a label; this measures what the INPUT does.  The unit is the read: a
 * window handed over as its occupied rows (c3_predict_rows) has n = row_count[b] reads, and variant j of it is the window without row j of
 * its run.  The device builds the n variants of every window from the rows staged once, runs them through the unchanged forward pass beside
 * the window itself -- the forms the handle is on: its plan, C3HIP_FP32, its calibration -- and reduces their rows to one record per window.
 * An instrument like c3_predict_exact, not a path of a pipeline: blocking, in the first lane, and nothing is allocated, launched or planned
 * unless one of these entries is called.
 * The definitions (clair3_amd/csrc/c3_jackknife.h; in numpy: synthetic.leave_one_out / jackknife_records), y the window's own row:
 *   layout      C3_JACKKNIFE_RECENTRE: the n - 1 rows that stay start at dense row (depth - (n - 1)) / 2 -- the reference's padding rule
 *               (row_first == NULL above) applied to the variant's own count, the window its producer would have laid out without that read.
 *               C3_JACKKNIFE_IN_PLACE: they start at the base window's first row.  The base window sits where row_first / the centring rule
 *               puts it, exactly as in c3_predict_rows.  A row of the run is a read whatever it holds: an interior all-zero row is a variant too;
 *               n = 1 has one variant, the all-zero window; n = 0 gives the all-zero record with lean_read = -1
 *   arg-max     of a head (21 | 3 | 33 | 33 columns): the first maximum by `>` from -inf on -- the lowest index on ties, a NaN never, the head's
 *               first column when nothing exceeds -inf: the rule of the census and of refine mode
 *   a NaN       or an infinity among a variant's probabilities: the variant counts in `nonfinite` and, by the arg-max rule, in flips and
 *               decision_flips; it is left out of lean_read / lean_drop and of max_delta.  A drop that is a NaN (the base row's own value is
 *               one) is never the largest; a zero drop that leans is reported as +0 */
#define C3_JACKKNIFE_RECENTRE 0
#define C3_JACKKNIFE_IN_PLACE 1
typedef struct c3_jackknife_window {   /* 80 bytes */
    int32_t reads;              /* n */
    int32_t nonfinite;          /* variants with a non-finite probability in their first nout columns */
    int32_t flips[4];           /* per head h: variants whose arg-max in h differs from the base row's (heads the model lacks: 0) */
    int32_t decision_flips[4];  /* rows with decoder columns: per reference base A C G T, variants whose decoder column 23 + b differs
                                   from the base row's; without decoder columns: 0 */
    int32_t lean_read[4];       /* per head: the j with the largest drop = y[t] - v_j[t], t the base arg-max of the head;
                                   lowest j on ties; -1 when no variant is finite (and for a head the model lacks) */
    float   lean_drop[4];       /* that drop (one float32 subtraction; may be negative); 0 with lean_read = -1 */
    float   max_delta;          /* max over finite variants and the first nout columns of |v_j[c] - y[c]| (float32) */
    int32_t reserved;
} c3_jackknife_window;
/* what a call did (the trailing argument of the two entries that run the network; may be NULL) */
typedef struct {
    int64_t windows, variants;  /* of the call */
    int64_t passes;             /* the call is cut into passes of C3HIP_JACKKNIFE_CHUNK windows (env; default 64, 0 = never cut) */
    int64_t bytes_staged;       /* host to device: the occupied rows and the tables */
    int32_t on_fp32;            /* 1: the range guard met a pass and that pass ran again on the fp32 forms (below) */
    int32_t reserved;
    float expand_us, reduce_us; /* device time of the call's jackknife_expand_kernel / jackknife_reduce_kernel launches (HIP events, summed) */
} c3_jackknife_info;
/*   c3_jackknife_rows    the arguments of c3_predict_rows.  Cut into passes of C3HIP_JACKKNIFE_CHUNK windows; a window's variants never
 *                        straddle a pass, they may straddle a micro-batch of 2048 dense windows.  Per pass the occupied rows and one table
 *                        (the windows themselves first, then every window's variants in window order, read order) are staged once, the dense
 *                        windows are built micro-batch by micro-batch in front of the forward pass, the rows stay in a buffer of the handle,
 *                        the reduction runs behind the last micro-batch and the host waits once, for the records.
 *                          y_host            (may be NULL) [batch][row]: bit for bit c3_predict_rows of the same arguments
 *                          out               [batch] records
 *                          drops_out         (may be NULL) [sum(row_count)][4] float32: y[t_h] - v_j[t_h] per variant and head (0: no such head)
 *                          variant_rows_out  (may be NULL) [sum(row_count)][row]: the variants' rows, for tests and tools
 *                        The handle is left as it was: c3_model_describe, the tap buffers of the last call, a profile being taken, the totals
 *                        of verify / refine / score mode and rows_windows= do not see the call.  Range guard: a handle on the fp16x3 forms whose
 *                        range flag is up behind a pass (or that returned a non-finite row) runs THAT PASS again on the fp32-MFMA forms for this
 *                        call alone; the device flag is put back to zero, the handle stays on its forms, info->on_fp32 says so.
 *   c3_jackknife         dense int8 windows: every window's run is found on the host as c3_pack_rows finds it, its first row is the run's own.
 *   c3_jackknife_reduce  the reduction alone on rows the caller holds (row_floats == c3_model_output_size(), or that + C3_DECODE_COLS):
 *                        base_rows [batch][row_floats], variant_rows [sum(row_count)][row_floats].  Needs no weights; serves both kinds.
 * Refused before anything is queued: a pileup handle and a handle without weights (the two entries that run the network), null buffers with
 * batch > 0, a negative count, first < 0, first + count > depth, a layout other than the two, a submit pending on any slot of the ring, a
 * handle that answers from the exact form (c3_model_set_answer), row_floats that is neither of the two.  batch == 0 launches nothing. */
int c3_jackknife_rows(c3_model *m, const void *rows_host, const int32_t *row_first, const int32_t *row_count, int64_t batch, int layout,
                      float *y_host, c3_jackknife_window *out, float *drops_out, float *variant_rows_out, c3_jackknife_info *info);
int c3_jackknife(c3_model *m, const void *x_host, int x_dtype, int64_t batch, int layout, float *y_host, c3_jackknife_window *out,
                 float *drops_out, float *variant_rows_out, c3_jackknife_info *info);
int c3_jackknife_reduce(c3_model *m, const float *base_rows, const float *variant_rows, int row_floats, const int32_t *row_count,
                        int64_t batch, c3_jackknife_window *out, float *drops_out);

/* ---- subsample mode: full-alignment calls under random read subsampling ("Subsample mode") ----
 * Jackknife mode takes ONE read away; this asks at what coverage a call holds.  A window handed over as its occupied rows has n =
 * row_count[w] reads.  The call names `levels` target depths D_0 < .. < D_{L-1} (1 <= L <= 8, every D >= 1), `replicates` R (1 <= R <= 32)
 * and a seed; for every level with D_l < n the device builds R variants of the window, each keeping D_l of its reads -- the subsets are
 * decided ON THE DEVICE from a stateless counter hash --, runs them through the unchanged forward pass beside the window itself (the forms
 * the handle is on) and reduces their rows to one record per (window, level) and one per window.  An instrument like jackknife mode:
 * blocking, in the first lane, and nothing is allocated, launched or planned unless one of these entries is called.
 * The rule (clair3_amd/csrc/c3_subsample.h states it once; in numpy: synthetic.subsample_keys / subsample_masks / subsample_variants /
 * subsample_records), w the window's index in the CALL:
 *   keys        key(w, r, j) = mix(seed + 0x9E3779B97F4A7C15 * (1 + (w * R + r) * depth + j)) mod 2^64, mix the SplitMix64 finaliser; the
 *               key does not depend on the level, so a replicate's subsets are nested
 *   selection   k = min(n, D_l); k == n: the level is not run for that window (it holds by definition); k < n: replicate r keeps the k reads
 *               of smallest (key, j), in read order.  Without replacement
 *   layout      C3_JACKKNIFE_RECENTRE: the kept rows start at dense row (depth - k) / 2; C3_JACKKNIFE_IN_PLACE: at the base window's first row
 *   order       of the variants: window by window, level by level (only levels that ran), replicate by replicate
 *   a NaN       or an infinity among a variant's probabilities: the variant counts in `nonfinite` and, by the arg-max rule of jackknife
 *               mode, in flips and decision_flips; it is left out of min_kept */
typedef struct c3_subsample_level {    /* 48 bytes; [batch][levels] */
    int32_t keep;               /* k = min(n, D_l) */
    int32_t run;                /* R, or 0 when k == n */
    int32_t nonfinite;          /* variants with a non-finite probability in their first nout columns */
    int32_t decision_flips;     /* rows with decoder columns: variants in which any of the decoder columns 23 .. 26 differs from the base
                                   row's; without decoder columns: 0 */
    int32_t flips[4];           /* per head h: variants whose arg-max in h differs from the base row's (heads the model lacks: 0) */
    float   min_kept[4];        /* per head: min over the level's finite variants of v[t_h], t_h the base arg-max of the head; the bits of
                                   the base row's y[t_h] when no finite variant ran; 0 for a head the model lacks */
} c3_subsample_level;
typedef struct c3_subsample_window {   /* 32 bytes */
    int32_t reads;              /* n */
    int32_t levels_run;
    int32_t hold_level[4];      /* per head: the lowest level index l with flips[h] == 0 at l and at every deeper level (levels that did not
                                   run hold); `levels` when the deepest level itself flips; 0 for a head the model lacks */
    int32_t hold_decision;      /* the same over decision_flips */
    int32_t reserved;
} c3_subsample_window;
/* what a call did (the trailing argument of the two entries that run the network; may be NULL) */
typedef struct {
    int64_t windows, variants;  /* of the call */
    int64_t passes;             /* the call is cut into passes of C3HIP_SUBSAMPLE_CHUNK windows (env; default 64, 0 = never cut) */
    int64_t bytes_staged;       /* host to device: the occupied rows and the tables */
    int32_t on_fp32;            /* 1: the range guard met a pass and that pass ran again on the fp32 forms */
    int32_t reserved;
    float expand_us, reduce_us; /* device time of the call's subsample_expand_kernel / subsample_reduce_kernel launches (HIP events, summed) */
} c3_subsample_info;
/*   c3_subsample_rows    the window arguments of c3_predict_rows.  Cut into passes of C3HIP_SUBSAMPLE_CHUNK windows (read at every call); a
 *                        window's variants never straddle a pass, and because the hash uses the call's window index the results do not
 *                        depend on the cut.  Per pass the occupied rows and one table are staged once, the dense windows are built
 *                        micro-batch by micro-batch in front of the forward pass, the reduction runs behind the last one and the host waits
 *                        once, for the records.
 *                          y_host            (may be NULL) [batch][row]: bit for bit c3_predict_rows of the same arguments
 *                          out               [batch] window records;  levels_out  [batch][levels] level records
 *                          masks_out         (may be NULL) [variants][2] uint64: bit j of the pair = read j kept
 *                          variant_rows_out  (may be NULL) [variants][row]: the variants' rows, for tests and tools
 *                        The handle is left as it was, and the range guard behaves as in c3_jackknife_rows: a pass beyond the fp16 range runs
 *                        again on the fp32-MFMA forms for this call alone, info->on_fp32 says so.
 *   c3_subsample         dense int8 windows: every window's run is found on the host as c3_jackknife finds it.
 *   c3_subsample_reduce  the reduction alone on rows the caller holds (row_floats == c3_model_output_size(), or that + C3_DECODE_COLS):
 *                        base_rows [batch][row_floats], variant_rows [variants][row_floats] in the rule's order.  Needs no weights; serves
 *                        both kinds.
 * Refused before anything is queued: a null model; a pileup handle, a handle without weights, a handle deeper than 128 rows (the two
 * entries that run the network); a submit pending on any slot of the ring; a handle that answers from the exact form; a layout other than
 * the two; levels outside 1 .. 8; depths not strictly increasing or below 1; replicates outside 1 .. 32; a negative count, first < 0,
 * first + count > depth; null required buffers; row_floats that is neither of the two.  batch == 0 launches nothing. */
int c3_subsample_rows(c3_model *m, const void *rows_host, const int32_t *row_first, const int32_t *row_count, int64_t batch,
                      const int32_t *depths, int levels, int replicates, uint64_t seed, int layout, float *y_host, c3_subsample_window *out,
                      c3_subsample_level *levels_out, uint64_t *masks_out, float *variant_rows_out, c3_subsample_info *info);
int c3_subsample(c3_model *m, const void *x_host, int x_dtype, int64_t batch, const int32_t *depths, int levels, int replicates,
                 uint64_t seed, int layout, float *y_host, c3_subsample_window *out, c3_subsample_level *levels_out, uint64_t *masks_out,
                 float *variant_rows_out, c3_subsample_info *info);
int c3_subsample_reduce(c3_model *m, const float *base_rows, const float *variant_rows, int row_floats, const int32_t *row_count,
                        int64_t batch, const int32_t *depths, int levels, int replicates, c3_subsample_window *out,
                        c3_subsample_level *levels_out);

/* ---- occlusion mode: which channels and which columns a call leans on, for both networks ("Occlusion mode") ----
 * Jackknife and subsample mode say what the READS do to a label; they refuse a pileup handle, whose windows hold counts.  This instrument
 * is on the input side of BOTH networks: for every window of a call the device builds K variants from the window staged once -- the window
 * with one channel set to zero, the window with one band of columns set to zero --, runs them through the unchanged forward pass beside the
 * window itself -- the forms the handle is on: its plan, C3HIP_FP32, its calibration -- and reduces their rows to one record per window plus
 * the complete map of drops.  Blocking, in the first lane, and nothing is allocated, launched or planned unless one of these entries is
 * called.
 * The definitions (clair3_amd/csrc/c3_occlude.h; in numpy: synthetic.occlude_variants / occlude_records).  A window has P positions and C
 * channels, the handle's geometry: full alignment (depth, P, C) int8, pileup (P, C) int8 or int32.  A call names `what`
 * (C3_OCCLUDE_CHANNELS = 1, C3_OCCLUDE_BANDS = 2, both = 3) and `band` (1 <= band <= P, columns per band); nb = ceil(P / band), band k
 * covers the columns [k * band, min(P, (k + 1) * band)).
 *   variants    every window of the call has the same K = (C if channels) + (nb if bands) variants, in this order: group 0, when channels
 *               are asked for: variant c (0 <= c < C) is the window with channel c set to zero at every position, and in every read for full
 *               alignment; group 1, when bands are asked for: variant k (0 <= k < nb) is the window with every channel of band k's columns
 *               set to zero, in every read.  Everything else stays where it is: a full-alignment variant keeps the base window's run where
 *               row_first / the centring rule puts it -- a read is not removed, so nothing is laid out again.  Window b's variants are the
 *               call's variants b * K .. b * K + K - 1.  A window without reads, or an all-zero window, still has K variants: all of them
 *               the zero window
 *   arg-max     of a head (21 | 3 | 33 | 33 columns): the first maximum by `>` from -inf on -- the lowest index on ties, a NaN never, the
 *               head's first column when nothing exceeds -inf: the rule of the census, of refine mode and of jackknife mode
 *   drop        of variant j in head h: y[t_h] - v_j[t_h] in one float32 subtraction, t_h the arg-max of the window's own row y in the head;
 *               0 for a head the model lacks
 *   a NaN       or an infinity among a variant's first nout columns: the variant counts in `nonfinite` and, by the arg-max rule, in flips
 *               and decision_flips; it is left out of lean / lean_drop and of max_delta.  A drop that is a NaN (the base row's own value is
 *               one) is never the largest; a zero drop that leans is reported as +0 */
#define C3_OCCLUDE_CHANNELS 1
#define C3_OCCLUDE_BANDS 2
typedef struct c3_occlude_window {        /* 144 bytes; [g]: group 0 = channels, group 1 = bands */
    int32_t variants;                 /* K */
    int32_t nonfinite;                /* variants with a non-finite value in their first nout columns */
    int32_t flips[2][4];              /* [g][h]: variants of group g whose arg-max in head h differs from y's, non-finite ones included
                                         (0 for a head the model lacks and for a group that was not asked for) */
    int32_t decision_flips[2][4];     /* [g][r]: rows with decoder columns: variants of group g whose decoder column 23 + r compares
                                         unequal to y's, r = A C G T; without decoder columns: 0 */
    int32_t lean[2][4];               /* [g][h]: the index within group g (the channel c, or the band k) of the largest drop among the
                                         finite variants whose drop is not a NaN, the lowest index on ties; -1 when there is none or the
                                         group was not asked for */
    float   lean_drop[2][4];          /* that drop (may be negative); 0 with lean = -1 */
    float   max_delta;                /* max over finite variants and the first nout columns of |v_j[c] - y[c]| (float32), NaN
                                         differences left out; 0 without any */
    int32_t reserved;
} c3_occlude_window;
/* what a call did (the trailing argument of the two entries that run the network; may be NULL) */
typedef struct {
    int64_t windows, variants;  /* of the call */
    int64_t passes;             /* the call is cut into passes of C3HIP_OCCLUDE_CHUNK windows (env, read at every call; default 64
                                   full-alignment windows, 256 pileup windows; 0 = never cut) */
    int64_t bytes_staged;       /* host to device: the occupied rows (full alignment) or the windows (pileup), and the tables */
    int32_t on_fp32;            /* 1: the range guard met a pass and that pass ran again on the fp32 forms (below) */
    int32_t reserved;
    float expand_us, reduce_us; /* device time of the call's occlude_*expand_kernel / occlude_reduce_kernel launches (HIP events, summed) */
} c3_occlude_info;
/*   c3_occlude         dense windows of either kind.  Full alignment: every window's run is found on the host as c3_jackknife finds it and
 *                      only the occupied rows are staged; pileup: the windows are staged as they are, int8 or int32 on their own kernels.
 *                      Cut into passes of C3HIP_OCCLUDE_CHUNK windows; a window's variants never straddle a pass, they may straddle a
 *                      micro-batch (2048 full-alignment, 16384 pileup dense windows); results do not depend on the cut.  Per pass the input
 *                      and one table (the windows themselves first, then every window's K variants in window order, variant order) are
 *                      staged once, the dense windows are built micro-batch by micro-batch in front of the forward pass, the rows stay in a
 *                      buffer of the handle, the reduction runs behind the last micro-batch and the host waits once, for the records.
 *                        y_host            (may be NULL) [batch][row]: bit for bit c3_predict / c3_predict_rows of the same arguments
 *                        out               [batch] records
 *                        drops_out         (may be NULL) [batch][K][4] float32: the map -- the drop of every variant in every head
 *                        variant_rows_out  (may be NULL) [batch][K][row]: the variants' rows, for tests and tools
 *                      The handle is left as it was: c3_model_describe, the tap buffers of the last call, a profile being taken, the totals
 *                      of verify / refine / score mode and rows_windows= do not see the call.  Range guard (full alignment): a handle on
 *                      the fp16x3 forms whose range flag is up behind a pass (or that returned a non-finite row) runs THAT PASS again on
 *                      the fp32-MFMA forms for this call alone; the device flag is put back to zero, the handle stays on its forms,
 *                      info->on_fp32 says so.  A pileup handle has no such guard.
 *   c3_occlude_rows    full alignment only: the arguments of c3_predict_rows.
 *   c3_occlude_reduce  the reduction alone on rows the caller holds (row_floats == c3_model_output_size(), or that + C3_DECODE_COLS):
 *                      base_rows [batch][row_floats], variant_rows [batch][channels + bands][row_floats]; `channels` and `bands` are the
 *                      sizes of the two groups, either may be 0.  Needs no weights; serves both kinds.
 * Refused before anything is queued: a submit pending on any slot of the ring, a handle that answers from the exact form
 * (c3_model_set_answer), a handle without weights (the two entries that run the network), null buffers with batch > 0, `what` outside
 * 1 .. 3, `band` outside 1 .. P, a dtype the kind does not take (full alignment int8; pileup int8 or int32), c3_occlude_rows on a pileup
 * handle, a negative count, first < 0, first + count > depth, a pass of more than INT32_MAX dense windows, row_floats that is neither of
 * the two, a negative group size.  batch == 0 launches nothing. */
int c3_occlude(c3_model *m, const void *x_host, int x_dtype, int64_t batch, int what, int band, float *y_host, c3_occlude_window *out,
               float *drops_out, float *variant_rows_out, c3_occlude_info *info);
int c3_occlude_rows(c3_model *m, const void *rows_host, const int32_t *row_first, const int32_t *row_count, int64_t batch, int what,
                    int band, float *y_host, c3_occlude_window *out, float *drops_out, float *variant_rows_out, c3_occlude_info *info);
int c3_occlude_reduce(c3_model *m, const float *base_rows, const float *variant_rows, int row_floats, int channels, int bands,
                      int64_t batch, c3_occlude_window *out, float *drops_out);

/* ---- gVCF mode: the non-variant half of the reference's --gvcf, the <NON_REF> block records, from the per-site counts of the pileup
 * step.  No c3_model is involved.  The rule, the argument why it is a chain of range queries, and the kernels: csrc/c3_gvcf.h.
 * One contig per call; a depth of at most 65535; at most INT32_MAX - 1024 sites a call.
 *   c3_gvcf_config   what variantInfoCalculator takes (preprocess/utils.py:350): p_err, gq_bin_size, bp_resolution
 *   c3_gvcf_block    one written record (write_to_gvcf_batch :577-606): a block, or one item of a block that the reference writes item by
 *                    item (per_site = 1: a ./. block, or any block under bp_resolution, whose first item's base is in ACGT)
 *   c3_gvcf_site     reference_likelihood / _cal_reference_likelihood (:490-568) of one site, plain host code:
 *                    out6 = gq, binned_gq, validPL (1: 0/0, 0: ./.), PL[3].  ref_byte is the raw reference byte: anything outside
 *                    upper-case ACGT gives gq = binned_gq = 1 and PL 0,0,0
 *   c3_gvcf_site_table  the same for every pair n_ref <= n_total <= depth with an ACGT base: out[6 * (n_total * (n_total + 1) / 2 + n_ref)]
 *   c3_gvcf_blocks_host  make_gvcf_online (:398-488) and the closing write_to_gvcf_batch of the producer (preprocess/
 *                    CreateTensorPileupFromCffi.py:419-437) over n_sites sites, sequentially on the host: needs no device.  Site j is
 *                    position first_pos + j; n_ref / n_total [n_sites] are C3_DTYPE_I32 or C3_DTYPE_I64 (= pos_ref_count /
 *                    pos_total_count themselves); ref_bytes [n_sites] raw reference bytes
 *   c3_gvcf_create / c3_gvcf_destroy   a device context: a stream, workspaces that grow and never shrink, the table of site records
 *   c3_gvcf_blocks_counts   the same records as c3_gvcf_blocks_host, on the device
 *   c3_gvcf_blocks_region   the same from the region matrix calculate_clair3_pileup returns (src/clair3_pileup.c:355-371, :452-455 undone
 *                    on the device): region_host (n_cols, 18) C3_DTYPE_I32 or C3_DTYPE_I64 (= plp_data.matrix), major_host = plp_data.major
 *                    (strictly increasing, 0-based); site j takes the column whose major is first_major + j, a site without a column has
 *                    0 / 0.  For the site the producer prints as P, the major is P when the chunk's ctg_start is not 1, P - 1 when it is
 *                    (CreateTensorPileupFromCffi.py:413-423)
 *   c3_gvcf_text     the lines of write_to_gvcf (:608-622) for a call's records, with its contig-end rule (END == contig_len - 1 prints
 *                    contig_len; contig_len <= 0: the contig is not in the header).  n_sites > 0 turns the producer's empty-pileup rule on
 *                    (CreateTensorPileupFromCffi.py:417-421, :439-440): where every record has max_dp 0, the one line of
 *                    write_empty_pileup (:392-397) stands in their place, pos max(1, first_pos), END first_pos + n_sites.  n_sites == 0
 *                    prints the records as they are, all-zero ones included (what make_gvcf_online itself writes for them)
 *   c3_gvcf_tile_sites / c3_gvcf_top_span / c3_gvcf_table_depth   constants of the device path, for tests: sites per tile, sites per
 *                    group of tiles (the last level that is walked one thread per group), rows of the device's record table
 * Sites deeper than the table's 1024 rows (up to 65535) cost a call one copy of its counts back to the host (4 bytes a site) and a side
 * table of the distinct deep pairs.
 * Status: 0; 1 with c3_last_error (a negative count, n_ref > n_total, a depth above 65535, null buffers, a dtype other than the two);
 * C3_GVCF_MORE when max_blocks (or buf_bytes) is too small: the count needed is in *n_blocks_out (*bytes_out), the first max_blocks records
 * are written and nothing beyond them (the text: nothing).  n_sites == 0 launches nothing and gives no record. */
#define C3_GVCF_MORE 2
typedef struct {
    double base_err;       /* --base_err, 0.001 */
    int32_t gq_bin_size;   /* --gq_bin_size, 5 */
    int32_t bp_resolution; /* --bp_resolution */
} c3_gvcf_config;
typedef struct c3_gvcf_block { /* 48 bytes */
    int64_t pos, end;       /* POS and END (before the contig-end rule of the text) */
    int32_t min_dp, max_dp; /* of the block's n_total; an item: its own */
    int32_t gq;             /* what is printed as GQ: the block's minimum of the items' gq; an item: its binned_gq; 1 when first_n */
    int32_t pl[3];
    uint8_t ref;            /* the printed base: A C G T or N */
    uint8_t gt;             /* 1: 0/0, 0: ./. */
    uint8_t per_site;       /* 1: an item of a block written item by item */
    uint8_t first_n;        /* 1: a block whose first item's base is outside ACGT (./., GQ 1, PL 0,0,0) */
    int32_t reserved;
} c3_gvcf_block;
typedef struct c3_gvcf c3_gvcf;
int c3_gvcf_site(const c3_gvcf_config *cfg, int64_t n_ref, int64_t n_total, int ref_byte, int32_t *out6);
int c3_gvcf_site_table(const c3_gvcf_config *cfg, int depth, int32_t *out);
int c3_gvcf_blocks_host(const c3_gvcf_config *cfg, const void *n_ref, const void *n_total, int dtype, const void *ref_bytes, int64_t n_sites,
                        int64_t first_pos, c3_gvcf_block *blocks_out, int64_t max_blocks, int64_t *n_blocks_out);
c3_gvcf *c3_gvcf_create(int device, const c3_gvcf_config *cfg);
int c3_gvcf_destroy(c3_gvcf *g);
int c3_gvcf_blocks_counts(c3_gvcf *g, const void *n_ref, const void *n_total, int dtype, const void *ref_bytes, int64_t n_sites, int64_t first_pos,
                          c3_gvcf_block *blocks_out, int64_t max_blocks, int64_t *n_blocks_out);
int c3_gvcf_blocks_region(c3_gvcf *g, const void *region_host, int x_dtype, int64_t n_cols, const int64_t *major_host, const void *ref_bytes,
                          int64_t first_major, int64_t n_sites, int64_t first_pos, c3_gvcf_block *blocks_out, int64_t max_blocks,
                          int64_t *n_blocks_out);
int c3_gvcf_text(const c3_gvcf_block *blocks, int64_t n_blocks, const char *ctg_name, int64_t contig_len, int64_t first_pos, int64_t n_sites,
                 char *buf, int64_t buf_bytes, int64_t *bytes_out);
int c3_gvcf_tile_sites(void);
int64_t c3_gvcf_top_span(void);
int c3_gvcf_table_depth(void);

/* ---- pileup from reads: the region matrix, its candidates with their alt-info, and the gVCF count pair of calculate_clair3_pileup
 * (src/clair3_pileup.c:208-461), from aligned reads as the arrays a BAM record holds.  No c3_model is involved and no file is read.
 * The rule clause by clause, where it deliberately leaves the reference, and the kernels: csrc/c3_pileup_rule.h, csrc/c3_pileup.h.
 *
 *   c3_read_set       host pointers in BAM's own encoding (bam1_core_t.pos / flag / qual, bam_get_cigar, bam_get_seq); reads in any order
 *   c3_pileup_config  calculate_clair3_pileup's arguments, and hash_mask: ANDed into the keys of the device's insertion table (all ones by
 *                     default; 0xF makes keys collide so that the fallback to the host form can be exercised).  gvcf == 0: no count pair
 *   c3_pileup_create / c3_pileup_destroy   a context: result buffers; with device >= 0 a stream and device buffers that grow and never shrink.
 *                     device < 0: a context without a GPU, for c3_pileup_reads_host alone
 *   c3_pileup_reads   the region [start, end), 0-based.  ref_bytes[i] is the reference at ref_first + i and must cover
 *                     [start, end + max_indel_length], else the call fails before anything is queued.  Limits of one call: 2^27 sites,
 *                     2^31 - 1 reads and CIGAR ops, 2^29 I and D ops in the kept reads, no CIGAR op of length 0.  hash_mask 0 counts
 *                     as all ones.  The result stays in the context
 *                     (matrix, major, candidate positions and depths on the device) until the next call
 *   c3_pileup_reads_host   the same rule as sequential host C; the result is held by the context on the host
 *   c3_pileup_sizes   of the held result: columns, candidates, sites of the count pair (end - start, or 0 without gvcf), bytes of text
 *   c3_pileup_result  copies the held result out; a null pointer skips that array.  matrix (n_cols, 18) int32, major (n_cols), candidate
 *                     positions (0-based) and depths (n_cand), n_ref / n_total (n_sites, indexed by p - start, 0 where no column exists), and
 *                     the alt-info text: one line per candidate, each closed by '\n', no terminating NUL
 *   c3_pileup_stats   of the last call.  fell_back: the device call found two different events under one key and answered through the host form
 *   c3_pileup_tile_sites   a constant of the device path, for tests: sites per compaction tile, which is also the tiles one step of the scan holds */
typedef struct c3_read_set {
    int64_t n_reads;
    const int64_t *pos;          /* [n] 0-based leftmost reference position */
    const uint16_t *flag;        /* [n] */
    const uint8_t *mapq;         /* [n] */
    const int64_t *cigar_first;  /* [n + 1] offsets into cigar */
    const uint32_t *cigar;       /* len << 4 | op, ops 0 .. 8 = MIDNSHP=X */
    const int64_t *seq_first;    /* [n + 1] byte offsets into seq */
    const uint8_t *seq;          /* 4-bit nt16 codes, two per byte, high nibble first, each read starting on a byte */
} c3_read_set;
typedef struct c3_pileup_config {
    int64_t min_depth;
    float min_snp_af, min_indel_af;
    int32_t min_mq, max_indel_length;
    int32_t call_snp_only, gvcf, call_ht, reserved;
    uint64_t hash_mask;
} c3_pileup_config;
typedef struct c3_pileup_counters {
    int64_t reads_kept, reads_dropped, events, collisions;
    int32_t fell_back, on_host;  /* on_host: the held result is the host form's (asked for, or fallen back to) */
    float kernel_ms[8];          /* device calls: op table, walk, indel table, reduce, site, compaction, staging in, fetch of the records */
} c3_pileup_counters;
typedef struct c3_pileup c3_pileup;
c3_pileup *c3_pileup_create(int device);
int c3_pileup_destroy(c3_pileup *p);
int c3_pileup_reads(c3_pileup *p, const c3_read_set *reads, int64_t start, int64_t end, const void *ref_bytes, int64_t ref_first, int64_t ref_len,
                    const c3_pileup_config *cfg);
int c3_pileup_reads_host(c3_pileup *p, const c3_read_set *reads, int64_t start, int64_t end, const void *ref_bytes, int64_t ref_first,
                         int64_t ref_len, const c3_pileup_config *cfg);
int c3_pileup_sizes(c3_pileup *p, int64_t *n_cols, int64_t *n_cand, int64_t *n_sites, int64_t *text_bytes);
int c3_pileup_result(c3_pileup *p, int32_t *matrix, int64_t *major, int64_t *cand_pos, int32_t *cand_depth, int64_t *n_ref, int64_t *n_total,
                     char *text);
int c3_pileup_stats(c3_pileup *p, c3_pileup_counters *out);
int c3_pileup_tile_sites(void);
/* The held result as a candidate batch of the ring: what c3_predict_submit_candidates / c3_predict_pileup_candidates compute from the arrays
 * c3_pileup_result returns (with the candidates' depths), rows, statuses and n_rows bit for bit, without the region matrix visiting the host:
 * it is copied from the context's device buffer into the slot on the lane's stream.  Context and model must be on one device.  A held
 * result of the host form (asked for, or fallen back to) is staged from the host like any other.  The submit fetches nothing from the
 * device.  The context's next c3_pileup_reads waits for the copy of the matrix, not for the batch; c3_predict_wait(m, slot) completes the
 * batch as usual. */
int c3_predict_submit_pileup(c3_model *m, c3_pileup *p, int head_tail, float *y_host, uint8_t *status_host, int64_t *n_rows_host, int slot);
int c3_predict_pileup_reads(c3_model *m, c3_pileup *p, int head_tail, float *y_host, uint8_t *status_host, int64_t *n_rows_host);

/* ---- full alignment from reads: the candidate windows of calculate_clair3_full_alignment (src/clair3_full_alignment_dwell.c:437-1054) from
 * aligned reads, as each window's occupied rows and a row count: what c3_predict_submit_rows with row_first == NULL takes (the dense window is
 * the run placed at (matrix_depth - count) / 2).  The rule clause by clause, every place where it deliberately leaves the reference, and the
 * kernels: csrc/c3_fa_rule.h, csrc/c3_fa_reads.h.  Limits: no BAM file is read; c3_fa_reads takes the haplotypes as an INPUT (c3_fa_reads_phased,
 * below, computes them from phased variants by the reference's haplotag_read); these entries build the 8-channel windows, c3_fa_reads_dwell
 * (further below) the 9-channel ones with the dwell channel; measured on synthetic reads only.
 *
 *   c3_read_extras    what a window needs beyond c3_read_set: one quality byte per query base (bam_get_qual; read r owns
 *                     qual[qual_first[r] .. qual_first[r + 1]), at least as many as its CIGAR consumes), the HP tag (0 unphased, 1, 2) and,
 *                     optionally, a 64-bit key of the read name for the duplicate-name filter (first occurrence wins; NULL: no filter)
 *   c3_fa_config      min_mq, max_indel_length (of the alt-info text), matrix_depth (89 or 55), seed (of the selection in windows with more
 *                     reads than matrix_depth), lds_reads: reads overlapping one candidate the device form handles (0: the kernel's table,
 *                     1024; a smaller value lowers it so that the fallback to the host form can be exercised)
 *   c3_fa_reads       centres: 0-based candidate positions, strictly ascending, each >= 16.  Reads must be in coordinate order.  ref_bytes[i]
 *                     is the reference at ref_first + i and must cover [centres[0] - 16, centres[last] + 16 + max_indel_length].  Returns 0;
 *                     C3_FA_ERR_REFSKIP when a kept read has an N op over a flanking position of a candidate; 1 for every other refusal; all
 *                     before anything is queued.  The result stays in the context (after a device call: rows, counts and centre depths on the
 *                     device) until the next call
 *   c3_fa_reads_host  the same rule as sequential host C; works in a context created with device < 0
 *   c3_fa_reads_sizes of the held result: candidates, rows (the sum of the counts), bytes of text, matrix_depth
 *   c3_fa_reads_result   copies the held result out; a null pointer skips that array.  rows (n_rows, 33, 8) int8 (33, 9 after c3_fa_reads_dwell), counts (n_cand) int32, centre
 *                     depths (n_cand) int32 (every kept read at the centre, not only the shown ones), the alt-info text: one line per candidate,
 *                     closed by '\n', no terminating NUL, entries in the order of c3_pileup_result's text (X, D by length, I by length then
 *                     bytes, R)
 *   c3_fa_reads_stats of the last call.  fell_back: a candidate had more overlapping reads than lds_reads and the host form answered
 *   c3_fa_lds_reads   a constant of the device path, for tests: the reads the candidate kernel's table holds (what lds_reads == 0 stands for) */
#define C3_FA_ERR_REFSKIP 2
typedef struct c3_read_extras {
    const int64_t *qual_first;   /* [n + 1] offsets into qual */
    const uint8_t *qual;
    const uint8_t *haplotype;    /* [n] 0, 1, 2 */
    const uint64_t *name_key;    /* [n] or NULL */
} c3_read_extras;
typedef struct c3_fa_config {
    int32_t min_mq, max_indel_length, matrix_depth, lds_reads;
    uint64_t seed;
} c3_fa_config;
typedef struct c3_fa_counters {
    int64_t reads_kept, reads_dropped, rows, deep_windows;  /* reads_dropped: by flag, mapq or name; deep_windows: more reads than matrix_depth */
    int32_t fell_back, on_host;
    float kernel_ms[8];  /* device calls: staging in, op table, candidates, scan, fill, fetch of the records; of a dwell call: moves staged
                          * (a part of the first), dwell table (a part of the second) */
} c3_fa_counters;
typedef struct c3_fa_reads_ctx c3_fa_reads_ctx;
c3_fa_reads_ctx *c3_fa_reads_create(int device);
int c3_fa_reads_destroy(c3_fa_reads_ctx *g);
int c3_fa_reads(c3_fa_reads_ctx *g, const c3_read_set *reads, const c3_read_extras *extras, const int64_t *centres, int64_t n_cand,
                const void *ref_bytes, int64_t ref_first, int64_t ref_len, const c3_fa_config *cfg);
int c3_fa_reads_host(c3_fa_reads_ctx *g, const c3_read_set *reads, const c3_read_extras *extras, const int64_t *centres, int64_t n_cand,
                     const void *ref_bytes, int64_t ref_first, int64_t ref_len, const c3_fa_config *cfg);
int c3_fa_reads_sizes(c3_fa_reads_ctx *g, int64_t *n_cand, int64_t *n_rows, int64_t *text_bytes, int32_t *matrix_depth);
int c3_fa_reads_result(c3_fa_reads_ctx *g, void *rows, int32_t *counts, int32_t *depths, char *text);
int c3_fa_reads_stats(c3_fa_reads_ctx *g, c3_fa_counters *out);
int c3_fa_lds_reads(void);
/* The held result as a rows batch of the ring: what c3_predict_submit_rows / c3_predict_rows compute from the rows and counts
 * c3_fa_reads_result returns (row_first == NULL), bit for bit, without the rows visiting the host: they are copied from the context's device
 * buffer into the slot on the lane's stream; the counts (which the call fetched anyway) make the slot's row table on the host.  n_rows_host
 * (may be NULL) receives the number of windows.  Context and model must be on one device; a held result of the host form is staged from
 * the host.  Refused before anything is queued: a pileup handle, a handle whose channel count is not the held result's (9 channels
 * against the 8 of c3_fa_reads, or 8 against the 9 of c3_fa_reads_dwell), a handle whose depth is not the result's matrix_depth.  The context's next c3_fa_reads waits for the copy, not for the batch; c3_predict_wait(m, slot) completes the batch. */
int c3_predict_submit_fa_reads(c3_model *m, c3_fa_reads_ctx *g, float *y_host, int64_t *n_rows_host, int slot);
int c3_predict_fa_reads(c3_model *m, c3_fa_reads_ctx *g, float *y_host, int64_t *n_rows_host);

/* ---- haplotagging the reads: the reference's haplotag_read (src/clair3_full_alignment_dwell.c:262-422, called at :629-632) as one host form
 * and one device form that give the same bytes, on their own (read tags out) and chained in front of the window kernels (the tags never
 * leave the device).  The rule clause by clause, its quirks and its one deviation: csrc/c3_hap_rule.h; the kernels: csrc/c3_hap_reads.h.
 * Limits: het SNPs only, as the reference; no VCF or BAM indexing; measured on synthetic read sets only.
 *
 *   c3_phased_variants   the phased heterozygous SNPs of ONE contig: pos 0-based and strictly ascending, alt_base a byte, genotype 1 (0|1)
 *                     or 2 (1|0), phase_set.  n == 0: every read is tagged 0
 *   c3_haplotag_config   min_haplotag_mq: reads below it are tagged 0 (the reference's constant is 20)
 *   c3_fa_haplotag    tags every read of the set (no flag or name filter; any read order) on the device; _host: the same rule as sequential
 *                     host C, works in a context created with device < 0.  ref_bytes[i] is the reference at ref_first + i and must cover
 *                     [v - 10, v + 11) of every variant v under a read that is tagged.  Refused with 1 and a message, before anything is
 *                     queued: null arrays, positions not strictly ascending, a genotype that is not 1 or 2, an uncovered context, and
 *                     what c3_pileup_reads refuses in a read set.  The tags stay in the context (after a device call: on the device) until
 *                     the next haplotag call
 *   c3_fa_haplotag_sizes   of the held tags: reads, (read, variant) pairs
 *   c3_fa_haplotag_result  copies out the tags hap (n_reads) and, for tests and diagnostics, the allele of every pair (0 none, 1 reference,
 *                     2 alternative) in read order, then variant order, with the n_reads + 1 offsets pair_first.  The pairs of a read: the
 *                     variants in [pos, end) (and at end when an I op stands there); a read below the mapq has none.  A null pointer skips
 *                     an array
 *   c3_fa_haplotag_stats   of the held tags (a device call's are counted when asked for, from one fetch)
 *   c3_fa_haplotag_shape   constants of the device path, for tests: pairs per workgroup of the pair kernel, pairs per step of the vote kernel
 *   c3_fa_reads_phased   c3_fa_haplotag and c3_fa_reads in one call: extras->haplotype is not read and may be NULL.  On the device the vote
 *                     kernel writes the array the window kernels read, on the context's stream, with no copy to the host in between; when
 *                     the window step falls back to its host form the tags are fetched once for it.  Refuses what either call refuses.
 *                     Afterwards c3_fa_reads_result / _sizes / _stats and c3_predict_submit_fa_reads work as after c3_fa_reads, and the
 *                     c3_fa_haplotag_* readers as after c3_fa_haplotag
 *   c3_fa_reads_phased_host   the same chain as sequential host C */
typedef struct c3_phased_variants {
    int64_t n;
    const int64_t *pos;         /* [n] 0-based, strictly ascending */
    const uint8_t *alt_base;    /* [n] */
    const uint8_t *genotype;    /* [n] 1 = 0|1, 2 = 1|0 */
    const int32_t *phase_set;   /* [n] */
} c3_phased_variants;
typedef struct c3_haplotag_config {
    int32_t min_haplotag_mq, reserved;
} c3_haplotag_config;
typedef struct c3_haplotag_counters {
    int64_t reads_hap[3];     /* reads tagged 0, 1, 2 (those below the mapq are among the 0s) */
    int64_t reads_low_mapq;
    int64_t pairs_realigned;  /* every pair of the offsets */
    int64_t pairs_allele0;
    int32_t on_host, reserved;
    float kernel_ms[8];       /* device calls: staging in, op table, pairs, votes; four unused */
} c3_haplotag_counters;
int c3_fa_haplotag(c3_fa_reads_ctx *g, const c3_read_set *reads, const c3_phased_variants *variants, const void *ref_bytes, int64_t ref_first,
                   int64_t ref_len, const c3_haplotag_config *cfg);
int c3_fa_haplotag_host(c3_fa_reads_ctx *g, const c3_read_set *reads, const c3_phased_variants *variants, const void *ref_bytes,
                        int64_t ref_first, int64_t ref_len, const c3_haplotag_config *cfg);
int c3_fa_haplotag_sizes(c3_fa_reads_ctx *g, int64_t *n_reads, int64_t *n_pairs);
int c3_fa_haplotag_result(c3_fa_reads_ctx *g, uint8_t *hap, int8_t *alleles, int64_t *pair_first);
int c3_fa_haplotag_stats(c3_fa_reads_ctx *g, c3_haplotag_counters *out);
int c3_fa_haplotag_shape(int32_t *pair_block, int32_t *vote_chunk);
int c3_fa_reads_phased(c3_fa_reads_ctx *g, const c3_read_set *reads, const c3_read_extras *extras, const c3_phased_variants *variants,
                       const int64_t *centres, int64_t n_cand, const void *ref_bytes, int64_t ref_first, int64_t ref_len,
                       const c3_fa_config *fa_cfg, const c3_haplotag_config *hap_cfg);
int c3_fa_reads_phased_host(c3_fa_reads_ctx *g, const c3_read_set *reads, const c3_read_extras *extras, const c3_phased_variants *variants,
                            const int64_t *centres, int64_t n_cand, const void *ref_bytes, int64_t ref_first, int64_t ref_len,
                            const c3_fa_config *fa_cfg, const c3_haplotag_config *hap_cfg);

/* ---- the dwell channel from move tables: the 9-channel windows of enable_dwell_time (src/clair3_full_alignment_dwell.c:20-74, :669-672,
 * :730-744, :905-911).  Channel 8 of a cell is the number of signal blocks the basecaller spent on the cell's base and on the insertions
 * attached to it, as (int8_t) of the int32 sum -- the reference's cast, no clamp (200 is stored as -56, 256 as 0).  The rule clause by
 * clause: csrc/c3_dwell_rule.h; the kernels: csrc/c3_dwell.h.  Channels 0 .. 7, counts, depths and text are those of c3_fa_reads.  Limits:
 * no BAM is read; the caller converts any `B` subtype of the mv tag to int8 (only zero or non-zero matters); synthetic tables only so far.
 *
 *   c3_read_moves     the `mv:B:c` tags of the reads of a c3_read_set, back to back: read r owns mv[mv_first[r] .. mv_first[r + 1]), element 0
 *                     of which is the stride and is skipped.  A read without the tag owns nothing
 *   c3_fa_reads_dwell c3_fa_reads with the dwell channel.  variants and hap_cfg are both NULL (the haplotypes come from extras, as
 *                     c3_fa_reads takes them) or both given (the call tags the reads first, as c3_fa_reads_phased does, and the tags stay on
 *                     the device).  Refused before anything is queued: a null moves, an mv_first that is negative or not non-decreasing,
 *                     only one of variants and hap_cfg, and whatever c3_fa_reads (and c3_fa_reads_phased) refuses.  Afterwards
 *                     c3_fa_reads_result returns rows (n_rows, 33, 9), and c3_predict_submit_fa_reads takes a 9-channel handle
 *   c3_fa_reads_dwell_host   the same rule as sequential host C; works in a context created with device < 0
 *   c3_fa_reads_channels     8 or 9: the channels of the held result's rows
 *   c3_fa_dwell_cum_host     the per-read rule on its own: cum_out[0 .. l] with cum_out[q] the sum of the signal lengths of the query bases
 *                     in front of q, in the order the BAM stores the bases (reverse != 0: a read with flag & 16); l: the read's quality
 *                     bytes.  Returns 1 when the read has a table, 0 when it has none (L <= 1 or l == 0; cum_out is then all zero)
 *   c3_fa_dwell_table the cum arrays of the last dwell call, read r at [qual_first[r] + r - qual_first[0] ..): qual_first[n] - qual_first[0]
 *                     + n int32, from the device after a device call.  Returns that number (0 when the last call was no dwell call), -1 on
 *                     an error; cum_out == NULL: nothing is copied
 *   c3_fa_dwell_step  a constant of the device path, for tests: the bytes of the staged tables one step of the table kernel covers.  The
 *                     steps of a read start at the 16-byte boundary at or in front of its table's first byte (the staged array starts at
 *                     mv_first[0]) */
typedef struct c3_read_moves {
    const int64_t *mv_first;  /* [n + 1] */
    const int8_t *mv;
} c3_read_moves;
int c3_fa_reads_dwell(c3_fa_reads_ctx *g, const c3_read_set *reads, const c3_read_extras *extras, const c3_read_moves *moves,
                      const c3_phased_variants *variants, const int64_t *centres, int64_t n_cand, const void *ref_bytes, int64_t ref_first,
                      int64_t ref_len, const c3_fa_config *fa_cfg, const c3_haplotag_config *hap_cfg);
int c3_fa_reads_dwell_host(c3_fa_reads_ctx *g, const c3_read_set *reads, const c3_read_extras *extras, const c3_read_moves *moves,
                           const c3_phased_variants *variants, const int64_t *centres, int64_t n_cand, const void *ref_bytes, int64_t ref_first,
                           int64_t ref_len, const c3_fa_config *fa_cfg, const c3_haplotag_config *hap_cfg);
int c3_fa_reads_channels(c3_fa_reads_ctx *g);
int c3_fa_dwell_cum_host(const int8_t *mv, int64_t L, int64_t l, int reverse, int32_t *cum_out);
int64_t c3_fa_dwell_table(c3_fa_reads_ctx *g, int32_t *cum_out);
int c3_fa_dwell_step(void);

/* Per-kernel-family HIP-event timing on the launch stream.  enable=1 brackets every kernel launch with
 * hipEvents (small overhead -- keep it off when measuring whole-job throughput). */
int c3_profile_enable(c3_model *m, int enable);
int c3_profile_reset(c3_model *m);
/* Fills up to max_entries records; returns the number of families, <0 on error.
 * flops are ALGORITHMIC (2*MACs of the reference layer shapes, no padding). */
typedef struct {
    char name[48];
    int64_t launches;
    double total_ms;
    double flops; /* summed over the recorded launches */
    double bytes; /* algorithmic bytes moved (inputs+outputs+weights once per launch) */
    double mfma_flops;       /* FLOP the matrix instructions EXECUTED (tile padding, fp16x3 piece products, Winograd reduction) */
    double mfma_peak_tflops; /* dense peak of the matrix instruction the family issues: 2500 (16-bit inputs) or 157.3 (fp32 inputs); 0 = no matrix work */
} c3_kernel_stat;
int c3_profile_read(c3_model *m, c3_kernel_stat *out, int max_entries);

#ifdef __cplusplus
}
#endif
#endif /* C3HIP_H */
