/*
 * fedavg_hip.h — C-ABI of libfedavg_hip.so, the MI355X (gfx950) FedAvg /
 * FedLesScan parameter-aggregation engine.
 *
 * The reference has no native code; its hot path is the numpy fold in
 *   fedless/aggregator/fed_avg_aggregator.py:24-42   FedAvgAggregator._aggregate
 *   fedless/aggregator/stall_aware_aggregation.py:42-67  StallAwareAggregator._aggregate
 * The Python drop-in classes (fedlesscan_amd/aggregator/) bind these entry
 * points with ctypes; INTEGRATION.md shows the binding a maintainer would add
 * to the reference itself.
 *
 * Conventions
 *  - Every data pointer is DEVICE memory (hipMalloc / torch CUDA tensors)
 *    unless marked [host].  The caller owns all buffers; the library never
 *    allocates or frees in a compute call.
 *  - X is row-major [N][ldx]: row i = client i's flattened parameters, in the
 *    order the reference iterates client_results.  ldx >= P (elements).
 *  - a[i] = fl(n_i), the client's cardinality rounded to the compute type the
 *    way numpy rounds a Python scalar; s[i] = fl((r_i+1)/(R+1)) for the
 *    stall-aware variant, NULL for FedAvg; divisor = fl(sum_i n_i) with the
 *    sum taken exactly (Python int).  These are [device] arrays of N.
 *  - stream is a hipStream_t (NULL = legacy default stream).  All work is
 *    enqueued on it; no call synchronises.  Calls are reentrant; the only
 *    state they keep is the measured kernel form per shape (fa_set_autotune),
 *    which changes which kernel runs, never the result.
 *  - Result, bit for bit:  acc = t_0; acc = acc + t_i (i = 1..N-1, in order);
 *    out = acc / divisor, where t_i = (x_i * a_i) [* s_i] with separate
 *    roundings (no FMA) and an IEEE divide.
 *  - Return FA_OK (0) or an FA_ERR_* code; fa_last_error() describes the last
 *    failure on the calling thread.
 */
#ifndef FEDAVG_HIP_H
#define FEDAVG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FA_ABI_VERSION 7

enum fa_status {
    FA_OK = 0,
    FA_ERR_ARG = 1,        /* bad size/pointer/stride -> ValueError                          */
    FA_ERR_NO_CLIENTS = 2, /* N == 0 -> InsufficientClientResults.  ABI guard only: the strategies never
                              fold zero rows (an empty round aggregates to [] on the host, as the
                              reference's _aggregate does: fed_avg_aggregator.py:31-42) */
    FA_ERR_SHAPE = 3,      /* -> InvalidParameterShapeError (exceptions.py:13)                  */
    FA_ERR_HIP = 4,        /* launch / runtime failure -> AggregationError (exceptions.py:1)    */
};

int fa_abi_version(void);
/* [host] message for the last failing call on this thread ("" if none). */
const char* fa_last_error(void);

/* ---- FedAvg / stall-aware fold over a stacked [N][ldx] matrix --------------
 * replaces FedAvgAggregator._aggregate      (fed_avg_aggregator.py:24-42)  when s == NULL
 * replaces StallAwareAggregator._aggregate  (stall_aware_aggregation.py:42-67) when s != NULL */
int fa_fedavg_f32(const float* X, int64_t N, int64_t P, int64_t ldx,
                  const float* a, const float* s, float divisor,
                  float* out, void* stream);

/* OPT-IN, NOT BIT-EXACT.  The same weighted mean for models too narrow to
 * fill the GPU (a few thousand to ~100K params): each column's clients are
 * cut into 32 contiguous slices folded in order, and the partial sums are
 * combined in a fixed pairwise tree (wavefront shuffles, then LDS).  Results
 * are deterministic run to run but differ from the reference's left fold
 * (fed_avg_aggregator.py:38-41) in the last bits: a different association
 * of the same sum.  Needs 16-B aligned X and out, ldx % 4 == 0. */
int fa_fedavg_f32_splitn(const float* X, int64_t N, int64_t P, int64_t ldx,
                         const float* a, const float* s, float divisor,
                         float* out, void* stream);

/* Same fold over N separately allocated client rows: xi is a [device] array of
 * N [device] pointers, each to P floats (the list-of-arrays form the reference
 * passes: fed_avg_aggregator.py:32-35). */
int fa_fedavg_f32_ptrs(const float* const* xi, int64_t N, int64_t P,
                       const float* a, const float* s, float divisor,
                       float* out, void* stream);
/* The same with every row promised 16-B aligned by the caller (and out 16-B
 * aligned): the tiled, grid-stride schedule of the stacked fold. */
int fa_fedavg_f32_ptrs_aligned(const float* const* xi, int64_t N, int64_t P,
                               const float* a, const float* s, float divisor,
                               float* out, void* stream);

/* Chunked fold, the building block of streaming ingest
 * (StreamFedAvgAggregator.aggregate, fed_avg_aggregator.py:111-153):
 *   acc_in == NULL : acc = t_0 + ... (as fa_fedavg_f32)
 *   acc_in != NULL : acc = acc_in[p] + t_0 + t_1 + ...  (continues a fold in order)
 *   finalize != 0  : out = acc / divisor, else out = acc (partial, unrounded by /)
 * acc_in may alias out.  Folding rows in chunks this way is bit-identical to
 * one fa_fedavg_f32 over all rows. */
int fa_fold_f32(const float* X, int64_t N, int64_t P, int64_t ldx,
                const float* a, const float* s, const float* acc_in,
                float divisor, int finalize, float* out, void* stream);

/* Single-row forms with scalar factors, for ingest that folds
 * each client as it arrives:
 *   fa_accumulate_f32: acc = first ? t : acc + t,  t = fl(fl(x*a) * s)
 *                      (s = 1.0f for FedAvg: multiplying by 1 is exact)
 *   fa_finalize_f32:   out = acc / divisor   (acc may alias out)
 * Accumulating the rows in client order and finalising once is bit-identical
 * to fa_fedavg_f32 over the stacked rows. */
int fa_accumulate_f32(float* acc, const float* x, float a, float s, int first, int64_t P, void* stream);
int fa_finalize_f32(const float* acc, float divisor, float* out, int64_t P, void* stream);

/* bf16 updates (BASELINE config 4; no reference path: defined as exact upcast
 * to f32 + the f32 fold).  out_f32 [P] (the fp32 result) and out_bf16 [P] (its
 * RNE bf16 copy) are each optional, at least one given (ABI 5: a multi-GPU
 * step exchanges only the bf16 copy, so it stores no fp32 result; both NULL ->
 * FA_ERR_ARG).  The bf16 bits are the same whether out_f32 is given or not. */
int fa_fedavg_bf16(const uint16_t* X, int64_t N, int64_t P, int64_t ldx,
                   const float* a, const float* s, float divisor,
                   float* out_f32, uint16_t* out_bf16, void* stream);

/* float16 updates (ABI 7).  The reference folds whatever dtype the clients
 * send: np.multiply(layer, n) with a Python-number weight keeps a float16 layer
 * float16 (NEP 50), so fed_avg_aggregator.py:31-41 and
 * stall_aware_aggregation.py:52-66 multiply, add and divide in binary16.  The
 * halves travel as their bit patterns; a, s [device, N halves] and divisor are
 * the factors already rounded to binary16 (s == NULL for FedAvg); out [P]:
 *   t_i = fl16(fl16(x_i * a_i) * s_i)       (FedAvg: t_i = fl16(x_i * a_i))
 *   acc = t_0;  acc = fl16(acc + t_i), i = 1..N-1 in client order
 *   out = fl16(acc / divisor)
 * Every operation is IEEE binary16 round-to-nearest-even with subnormals kept
 * and no FMA; factors that overflowed to inf stay inf, as in the reference.
 * NaN positions match numpy's, NaN sign and payload are unspecified.  Same
 * argument checks and status codes as fa_fedavg_f32.  16-B aligned X and out
 * with ldx % 8 == 0 take the vector forms (a measured form per shape, kind
 * FA_FOLD_F16), anything else one column per lane; out may overlap X. */
int fa_fedavg_f16(const uint16_t* X, int64_t N, int64_t P, int64_t ldx,
                  const uint16_t* a, const uint16_t* s, uint16_t divisor,
                  uint16_t* out, void* stream);

/* Chunked binary16 fold (new symbol, ABI still 7): fa_fold_f32's contract in
 * the arithmetic of fa_fedavg_f16, the building block of streaming ingest for
 * float16 models (the reference's aggregate() on float16 results,
 * fed_avg_aggregator.py:57-92, stall_aware_aggregation.py:82-117, folds them
 * in binary16: NEP 50).  acc_in and out are halves:
 *   acc_in == NULL : acc = t_0 (not 0 + t_0: a column of -0.0 stays -0.0)
 *   acc_in != NULL : acc = fl16(acc_in[p] + t_0), then t_1, ... in row order
 *   finalize != 0  : out = fl16(acc / divisor), the float32 divide of the
 *                    exactly converted operands rounded once; else out = acc
 *   N == 0 with acc_in: only the divide (or, without finalize, a copy)
 * acc_in may alias out.  Every add rounds to binary16 already, so the halves
 * carried between calls are the whole accumulator: folding the rows in any
 * cuts is bit-identical to one fa_fedavg_f16 over all of them.  Argument
 * checks and status codes as fa_fedavg_f16 (N == 0 without acc_in ->
 * FA_ERR_NO_CLIENTS); a capturing stream -> FA_ERR_ARG (no captured staging
 * carries binary16 factors).  One form fixed by shape (2 octets per lane, 4
 * rows ahead, balanced grid-stride passes); X, acc_in or out off 16-B alignment
 * or ldx % 8 != 0: one column per lane.  The kernels read the aligned 4-byte
 * word that holds each factor: a and s must each end on a 4-byte boundary
 * inside their allocation. */
int fa_fold_f16(const uint16_t* X, int64_t N, int64_t P, int64_t ldx,
                const uint16_t* a, const uint16_t* s, const uint16_t* acc_in,
                uint16_t divisor, int finalize, uint16_t* out, void* stream);

/* The 16-bit folds over N separately allocated client rows (new symbols, ABI
 * still 7): xi is a [device] array of N [device] pointers, each to P bf16 /
 * binary16 elements -- the list-of-arrays form the reference passes
 * (fed_avg_aggregator.py:32-35), folded where the rows lie, with no stacking
 * copy.  rows_aligned != 0 is the caller's promise that every row and every
 * given output is 16-B aligned and takes the octet kernels (a fixed form per
 * shape, not measured); with 0 rows and outputs may sit at any 2-B offset and
 * one lane folds a column.  Bit for bit the result of fa_fedavg_bf16 /
 * fa_fedavg_f16 over the same rows stacked, with either kernel.  Argument
 * checks and status codes as fa_fedavg_f32_ptrs and the stacked 16-bit folds
 * (both bf16 outputs NULL -> FA_ERR_ARG; rows_aligned != 0 with an output off
 * 16-B alignment -> FA_ERR_ARG).  The table lives in device memory, so the
 * library cannot see an alias: no output may overlap a row -- as the
 * reference, which returns new arrays. */
int fa_fedavg_bf16_ptrs(const uint16_t* const* xi, int64_t N, int64_t P,
                        const float* a, const float* s, float divisor, int rows_aligned,
                        float* out_f32, uint16_t* out_bf16, void* stream);
int fa_fedavg_f16_ptrs(const uint16_t* const* xi, int64_t N, int64_t P,
                       const uint16_t* a, const uint16_t* s, uint16_t divisor, int rows_aligned,
                       uint16_t* out, void* stream);

/* ---- one launch per exchange step (ABI 3) -----------------------------------
 * At N > 1 a rank folds its columns in `rounds` slots and all-gathers each
 * slot while the next one folds (fedlesscan_amd/sharding.py).  Folding each
 * slot in its own launch leaves a tail per launch, and the launches beside the
 * exchange lose blocks to the collective's kernels.  fa_fedavg_*_rounds folds
 * every slot of a step in ONE launch: column tiles are taken from a device
 * counter (round 0's first, then round 1's, ...), so a round's last tiles
 * overlap the next round's first ones and blocks that share a CU with other
 * kernels fold fewer tiles; when round k's last tile is done the launch
 * raises round k's flag.  fa_rounds_wait(r, k, stream) enqueues on another
 * stream a one-lane kernel that returns once round k of r's last launch is
 * complete (its results visible device-wide): the exchange of round k
 * enqueued behind it on that stream starts mid-launch.  Same bits as
 * fa_fedavg_f32 / fa_fedavg_bf16 on each slot.
 *   fa_rounds_create / _destroy: the launch state (device signal words) for
 *     one device; launches with one object must be ordered (one stream), and
 *     destroy synchronises the device.
 *   offsets [host] rounds + 1 local columns: round k folds columns
 *     [offsets[k], offsets[k+1]) of X (and writes the same columns of out);
 *     every round non-empty, 16-B aligned (offsets % 4, bf16 % 8), ldx too;
 *     1 <= rounds <= 8.  Not under graph capture (FA_ERR_ARG).
 *   fa_rounds_wait: round < the last launch's rounds; the stream first waits
 *     for the launch to reach the head of its own stream (an event recorded
 *     just before it), then a waiter that sees no completion within 30 s
 *     (FEDAVG_ROUND_WAIT_US at fa_rounds_create: another limit, for tests)
 *     returns anyway: whatever is queued behind it would read an unfinished
 *     round.  The waiter records that in page-locked host memory.
 *   fa_rounds_check (ABI 4): [host, no HIP call, no synchronisation] the
 *     number of rounds whose wait timed out in the launches since the last
 *     check (or creation), as far as the waits that have already run show --
 *     call it once the waits are known complete (an event recorded behind
 *     them); nonzero means an exchange behind a wait read an unfinished round
 *     and its result must not be used (fedlesscan_amd/sharding.py raises
 *     AggregationError on every rank).
 *   fa_rounds_timeouts: (synchronous) every timed-out wait since creation.
 *   fa_fedavg_bf16_rounds: out_f32 / out_bf16 as fa_fedavg_bf16 (ABI 5: either
 *     may be NULL, not both).
 *   out_offsets (ABI 5) [host] rounds output columns, or NULL: round k's
 *     results go to columns [out_offsets[k], out_offsets[k] + width k) of the
 *     outputs instead of [offsets[k], offsets[k+1]) (each 4-aligned, bf16
 *     8-aligned) -- a rank writes its slot of round k straight into its own
 *     chunk of the gathered model, and the all-gather runs in place. 
 *   One object per launching stream (engine.py keeps one per stream object). */
typedef struct fa_rounds fa_rounds;
int fa_rounds_create(fa_rounds** r, int device);
int fa_rounds_destroy(fa_rounds* r);
int fa_fedavg_f32_rounds(fa_rounds* r, const float* X, int64_t N, int64_t ldx,
                         const float* a, const float* s, float divisor, float* out,
                         int rounds, const int64_t* offsets, const int64_t* out_offsets, void* stream);
int fa_fedavg_bf16_rounds(fa_rounds* r, const uint16_t* X, int64_t N, int64_t ldx,
                          const float* a, const float* s, float divisor,
                          float* out_f32, uint16_t* out_bf16,
                          int rounds, const int64_t* offsets, const int64_t* out_offsets, void* stream);
int fa_rounds_wait(fa_rounds* r, int round, void* stream);
int fa_rounds_check(fa_rounds* r);
int fa_rounds_timeouts(fa_rounds* r);
/* [host] the kernel form fa_fedavg_bf16_rounds (bf16 != 0) / _f32_rounds runs */
const char* fa_rounds_form(int bf16);

/* The one launch per exchange step for float16 rows (new symbols, ABI still
 * 7): `_aggregate` of both strategies (fed_avg_aggregator.py:31-41,
 * stall_aware_aggregation.py:52-66) on a rank's slots of float16 layers, which
 * numpy folds in binary16 under Python-number weights -- the arithmetic of
 * fa_fedavg_f16, every round of a step in one launch as fa_fedavg_bf16_rounds.
 * Bit for bit fa_fedavg_f16 on each round's columns.  a, s [device, N halves]
 * and divisor are binary16 bit patterns as for fa_fedavg_f16 (s == NULL for
 * FedAvg); the kernels read the aligned 4-byte word that holds each factor, so
 * a and s must each end on a 4-byte boundary inside their allocation, as for
 * fa_fold_f16.  out [halves] receives round k at columns [offsets[k],
 * offsets[k+1]) or, with out_offsets, [out_offsets[k], ...).  offsets and
 * out_offsets % 8 == 0, 1 <= rounds <= 8, X and out 16-B aligned, ldx % 8 == 0;
 * a capturing stream -> FA_ERR_ARG.  The rounds are published at agent scope
 * (a state of fa_peers_rounds, whose rounds other GPUs read, -> FA_ERR_ARG).
 * fa_rounds_wait / _check / _timeouts serve it as they do the other two. */
int fa_fedavg_f16_rounds(fa_rounds* r, const uint16_t* X, int64_t N, int64_t ldx,
                         const uint16_t* a, const uint16_t* s, uint16_t divisor, uint16_t* out,
                         int rounds, const int64_t* offsets, const int64_t* out_offsets, void* stream);
/* [host] the kernel form fa_fedavg_f16_rounds runs */
const char* fa_rounds_form_f16(void);

/* The one launch per exchange step for float64 rows (new symbols, ABI still
 * 7): `_aggregate` of both strategies (fed_avg_aggregator.py:31-41,
 * stall_aware_aggregation.py:52-66) on a rank's slots of float64 layers -- the
 * dtype of the reference's own fixture (test/test_aggregation.py:23-38) -- in
 * the arithmetic of fa_fedavg_f64: t_i = fl64(fl64(x_i * a_i) * s_i), no FMA,
 * acc = t_0 then fl64(acc + t_i) in client order, the IEEE double divide,
 * subnormals kept.  Bit for bit fa_fedavg_f64 on each round's columns, every
 * round of a step in one launch as fa_fedavg_f32_rounds.  a, s [device, N
 * doubles] (s == NULL for FedAvg) and divisor as for fa_fedavg_f64.  out
 * [doubles] receives round k at columns [offsets[k], offsets[k+1]) or, with
 * out_offsets, [out_offsets[k], ...).  offsets and out_offsets % 2 == 0,
 * 1 <= rounds <= 8, X and out 16-B aligned, ldx % 2 == 0; a capturing stream
 * -> FA_ERR_ARG.  The rounds are published at agent scope (a state of
 * fa_peers_rounds, whose rounds other GPUs read, -> FA_ERR_ARG).
 * fa_rounds_wait / _check / _timeouts serve it as they do the other three. */
int fa_fedavg_f64_rounds(fa_rounds* r, const double* X, int64_t N, int64_t ldx,
                         const double* a, const double* s, double divisor, double* out,
                         int rounds, const int64_t* offsets, const int64_t* out_offsets, void* stream);
/* [host] the kernel form fa_fedavg_f64_rounds runs */
const char* fa_rounds_form_f64(void);

/* ---- kernel-free peer exchange of a step (ABI 4; ABI 5: no fence) ----------
 * The reference saves ONE global model per round (aggregation.py:125-138 ->
 * ParameterDao.save, client_daos.py:351-378); at N > 1 every rank folds its
 * slots and needs every other rank's.  An RCCL all-gather runs copy kernels on
 * a few CUs beside the next round's fold; here each rank PULLS its peers'
 * finished slots with hipMemcpyAsync on two copy streams from their send
 * buffers, opened once through IPC handles.  One object per rank and layout;
 * every call below that names a step is made by every rank of the group, in
 * the same order.
 *   fa_peers_create:  this rank's two send buffers (send_bytes each, a 16-B
 *                     multiple; step e's fold writes buffer e % 2) and its own
 *                     rounds state (device memory)
 *   fa_peers_handle_bytes / fa_peers_handle: [host] this rank's IPC handles
 *   fa_peers_open:    [host] every rank's handles, world x handle_bytes in rank
 *                     order (all-gathered by the caller); opens the peers'
 *   fa_peers_send:    [host] the send buffer of the NEXT fold launch with
 *                     fa_peers_rounds (ask before every step): the fold writes
 *                     this rank's slots there (out_bf16 for bf16 rows, out for fp32)
 *   fa_peers_rounds:  [host] the rounds state (owned by the fa_peers) to pass
 *                     to fa_fedavg_*_rounds: its launches store their tiles
 *                     system-coherent and publish every round at system scope,
 *                     and each waits for the state's previous exchange
 *   fa_peers_exchange: enqueue, after the launch, on another stream: per round
 *                     k, a wait until every rank has completed round k, then
 *                     rank q's bytes [src_offsets[k], src_offsets[k+1]) of its
 *                     send buffer of this step are copied to dst +
 *                     dst_offsets[k * world + q] (this rank's own slot
 *                     included, last).  A wait that gives up is reported by
 *                     fa_rounds_check(fa_peers_rounds).  The next fold launch
 *                     with the state waits for this exchange; with the two
 *                     buffers that is what keeps a buffer from being rewritten
 *                     before every peer has pulled it (no fence, no ack)
 *   fa_peers_destroy: after every rank's last exchange (a barrier) */
typedef struct fa_peers fa_peers;
int fa_peers_create(fa_peers** x, int device, int world, int rank, int64_t send_bytes);
int fa_peers_destroy(fa_peers* x);
int fa_peers_handle_bytes(void);
int fa_peers_handle(fa_peers* x, void* out);
int fa_peers_open(fa_peers* x, const void* all_handles);
void* fa_peers_send(fa_peers* x);
fa_rounds* fa_peers_rounds(fa_peers* x);
int fa_peers_exchange(fa_peers* x, int rounds, const int64_t* src_offsets, void* dst, const int64_t* dst_offsets,
                      void* stream);

/* The same folds with the per-client factors a[0..N), s[0..N) (s may be
 * NULL) in HOST memory, as the reference's caller holds them (Python numbers,
 * fed_avg_aggregator.py:32-41).  The library copies them into a page-locked
 * slot of its own, sends them in one async H2D on a staging stream of its own
 * that `stream` waits for (an event) ahead of the fold, and reuses the slot
 * only after that fold has completed, so a and s may be freed or rewritten as
 * soon as the call returns.  X, xi, out stay device
 * pointers.  _ptrs: rows_aligned != 0 takes fa_fedavg_f32_ptrs_aligned's
 * kernels (every row 16-B aligned, out 16-B aligned), 0 fa_fedavg_f32_ptrs. */
int fa_fedavg_f32_hostf(const float* X, int64_t N, int64_t P, int64_t ldx,
                        const float* a, const float* s, float divisor,
                        float* out, void* stream);
int fa_fedavg_f32_ptrs_hostf(const float* const* xi, int64_t N, int64_t P,
                             const float* a, const float* s, float divisor,
                             int rows_aligned, float* out, void* stream);
int fa_fedavg_bf16_hostf(const uint16_t* X, int64_t N, int64_t P, int64_t ldx,
                         const float* a, const float* s, float divisor,
                         float* out_f32, uint16_t* out_bf16, void* stream);
/* fa_fedavg_bf16_ptrs (the list-of-arrays form, fed_avg_aggregator.py:32-35)
 * with a and s in [host] memory, staged like the entries above: the bits of
 * fa_fedavg_bf16 over the same rows stacked; no output may overlap a row. */
int fa_fedavg_bf16_ptrs_hostf(const uint16_t* const* xi, int64_t N, int64_t P,
                              const float* a, const float* s, float divisor, int rows_aligned,
                              float* out_f32, uint16_t* out_bf16, void* stream);
/* The _hostf entries refuse a capturing stream (FA_ERR_ARG, ABI 6): a graph
 * would have to own the staged copy.  Under capture, write the factors into
 * memory the graph owns (PyTorch: a tensor allocated inside the capture) with
 * fa_factors_fill -- dst[0..N) = a, then dst[N..2N) = s when s != NULL, by
 * kernels whose arguments carry the values, so replays need no host memory --
 * and call the device-factor entry (fa_fedavg_f32, fa_fedavg_bf16, ...). */
int fa_factors_fill(float* dst, const float* a, const float* s, int64_t N, void* stream);
/* The one-launch step with host factors (ABI 5): as fa_fedavg_*_rounds, the
 * factors staged by the library like the folds above (one C call per step). */
int fa_fedavg_f32_rounds_hostf(fa_rounds* r, const float* X, int64_t N, int64_t ldx,
                               const float* a, const float* s, float divisor, float* out,
                               int rounds, const int64_t* offsets, const int64_t* out_offsets, void* stream);
int fa_fedavg_bf16_rounds_hostf(fa_rounds* r, const uint16_t* X, int64_t N, int64_t ldx,
                                const float* a, const float* s, float divisor,
                                float* out_f32, uint16_t* out_bf16,
                                int rounds, const int64_t* offsets, const int64_t* out_offsets, void* stream);

/* Measured form choice.  Every kernel form of the fp32, bf16, float16 and
 * row-table folds computes the same bits; which is fastest depends on how a shape's
 * tiles fall on the CUs.  For plain one-shot folds (fa_fedavg_f32, _bf16,
 * _f16, _f32_ptrs_aligned and the _hostf forms) the FIRST call of a new (device,
 * kind, N, P, ldx, scored) shape runs every candidate form on the caller's
 * data and stream (an untimed launch each, then two timed passes of batched
 * launches between events), and once those events have completed -- read
 * back without synchronising on later calls -- the shape runs the fastest
 * (the shape policy's own form unless another is > 3 % faster).  Outputs are
 * bit-identical whatever form runs.  Library-wide switch, on unless
 * FEDAVG_AUTOTUNE=0 at load; FEDAVG_AUTOTUNE_LOG=1 prints each decision.
 *   fa_set_autotune:     1 on, 0 off (the policy form only), -1 query;
 *                        returns the previous setting
 *   fa_autotune_pending: shapes seen whose measurement is not complete
 *   fa_fold_form:        the form a shape runs on the stream's device:
 *                        the measured choice, "" while it is being measured,
 *                        the policy's form for an unseen shape or with the
 *                        tuner off.
 * The measuring call runs several launches into the same output, so a fold
 * whose out overlaps its input rows keeps the policy's single launch; for
 * fa_fedavg_f32_ptrs_aligned (row pointers live in device memory) out must
 * not alias a row -- as the reference, which returns new arrays. */
enum fa_fold_kind {
    FA_FOLD_F32 = 1,      /* fa_fedavg_f32 (_hostf)                     */
    FA_FOLD_BF16 = 2,     /* fa_fedavg_bf16 (_hostf)                    */
    FA_FOLD_F32_ROWS = 3, /* fa_fedavg_f32_ptrs_aligned (_hostf), ldx = P */
    FA_FOLD_F16 = 4,      /* fa_fedavg_f16                              */
};
int fa_set_autotune(int mode);
int fa_autotune_pending(void);
const char* fa_fold_form(int kind, int64_t N, int64_t P, int64_t ldx, int scored, void* stream);
/* Decisions outlive the process (ABI 3).  A shape's key takes the client
 * count as its power-of-two bucket (a round with 1000 results reuses what
 * 1024 measured) plus the policy's form.  Every decision is merged into a
 * text cache file (one line per shape: device arch and CU count, ABI version,
 * kind, client bucket, policy form, P, ldx, scored, chosen form -- forms by
 * name), written under an exclusive lock through a temp file and a rename;
 * the first tuned call of a process reads it, so a cold process (one FaaS
 * invocation: aggregation.py:71-75) runs a known shape's form on its first
 * call.  Unparseable lines, another ABI or an unknown form are ignored.
 * Default path $XDG_CACHE_HOME/fedlesscan_amd/tuner.txt or
 * ~/.cache/fedlesscan_amd/tuner.txt; FEDAVG_TUNE_CACHE=<path> or =0 (off).
 *   fa_tune_cache_path: set the file at run time ("" or NULL: off)
 *   fa_tune_export:     [host] this process's decisions as those lines into
 *                       buf (NUL-terminated, truncated to cap - 1); returns
 *                       the full length
 *   fa_tune_import:     [host] apply such lines (a decision made elsewhere
 *                       replaces this process's own for the same shape);
 *                       returns the number of lines applied.  A multi-GPU job
 *                       broadcasts rank 0's export so that every rank runs the
 *                       same forms. */
int fa_tune_cache_path(const char* path);
int64_t fa_tune_export(char* buf, int64_t cap);
int fa_tune_import(const char* text);
/* Step-form decisions (ABI 4).  A multi-GPU exchange step runs as one
 * fa_fedavg_*_rounds launch or as one fold launch per round; which is faster
 * depends on how much the exchange's kernels slow the fold on the machine,
 * so ShardedAggregator measures it once (an opt-in probe) and keeps the
 * answer in the tuner's cache file as a "fedavg-step" line, exported and
 * imported with the kernel forms.  key = "<device identity> <f32|bf16>
 * <world size> <client-count bucket (a power of two)> <P> <w0,w1,...>" (the
 * layout's 1-8 slot widths).  A cold process then runs the recorded form with
 * no probe (aggregation.py:71-75 builds a fresh strategy per invocation).
 *   fa_step_lookup: 1 one launch per step, 0 per-round launches, -1 no
 *                   decision, -2 malformed key (the file is read once)
 *   fa_step_record: record (and merge into the file) a decision */
int fa_step_lookup(const char* key);
int fa_step_record(const char* key, int one_launch);

/* float64 updates (the reference unit-test fixture is float64,
 * test/test_aggregation.py:23-38). */
int fa_fedavg_f64(const double* X, int64_t N, int64_t P, int64_t ldx,
                  const double* a, const double* s, double divisor,
                  double* out, void* stream);

/* Chunked binary64 fold (new symbol, ABI still 7): fa_fold_f32's contract in
 * the arithmetic of fa_fedavg_f64, the building block of streaming ingest for
 * float64 models (numpy's default dtype; the reference's aggregate() on
 * float64 results, fed_avg_aggregator.py:57-92,
 * stall_aware_aggregation.py:82-117, and its own unit-test fixture,
 * test/test_aggregation.py:23-38):
 *   t_i = fl64(fl64(x_i * a_i) * s_i)       (s == NULL: t_i = fl64(x_i * a_i)); no FMA
 *   acc_in == NULL : acc = t_0 (not 0 + t_0: a column of -0.0 stays -0.0)
 *   acc_in != NULL : acc = fl64(acc_in[p] + t_0), then t_1, ... in row order
 *   finalize != 0  : out = fl64(acc / divisor), the IEEE divide, no reciprocal;
 *                    else out = acc
 *   N == 0 with acc_in: only the divide (or, without finalize, a copy)
 * acc_in may alias out.  Subnormals are kept, NaN by position.  Every add
 * rounds to binary64 already, so folding the rows in any cuts is bit-identical
 * to one fa_fedavg_f64 over all of them.  Argument checks and status codes as
 * fa_fedavg_f64 (N == 0 without acc_in -> FA_ERR_NO_CLIENTS).  One form fixed
 * by shape (4, 2 or 1 pairs of columns per lane by width, 4 rows ahead,
 * balanced grid-stride passes over at most one block per CU); X, acc_in or out
 * off 16-B alignment or an odd ldx: one column per lane. */
int fa_fold_f64(const double* X, int64_t N, int64_t P, int64_t ldx,
                const double* a, const double* s, const double* acc_in,
                double divisor, int finalize, double* out, void* stream);

/* The float64 fold over N separately allocated client rows (new symbol, ABI
 * still 7): xi is a [device] array of N [device] pointers, each to P doubles --
 * the list-of-arrays form the reference passes (fed_avg_aggregator.py:32-35),
 * folded where the rows lie, with no stacking copy.  rows_aligned != 0 is the
 * caller's promise that every row and out are 16-B aligned and takes the pair
 * kernel (a fixed form per shape, 8 rows ahead); with 0 rows and out may sit
 * at any 8-B offset and one lane folds a column.  Bit for bit the result of
 * fa_fedavg_f64 over the same rows stacked, with either kernel.  Argument
 * checks and status codes as fa_fedavg_f16_ptrs (rows_aligned != 0 with out
 * off 16-B alignment -> FA_ERR_ARG).  The table lives in device memory, so
 * the library cannot see an alias: out may not overlap a row. */
int fa_fedavg_f64_ptrs(const double* const* xi, int64_t N, int64_t P,
                       const double* a, const double* s, double divisor, int rows_aligned,
                       double* out, void* stream);

/* ---- every layer of a device-resident model in one launch (new symbols, ABI
 * still 7) -------------------------------------------------------------------
 * The reference folds a model layer by layer over the clients' lists of
 * arrays (fed_avg_aggregator.py:24-42: `layer * num_examples` per client and
 * layer, :32-35; reduce(np.add) and the divide per layer, :38-41).  The
 * row-table folds above take one layer per launch; these take all L layers:
 *   xi    [device] L*N row bases, layer-major: xi[l*N + i] = client i's layer l
 *   plan  [device] L entries (fa_layer_plan), as fa_layers_plan wrote them
 *   tiles, units  the tile total and the units per lane of that plan
 * One grid-stride launch over the `tiles` tiles of all layers, balanced passes
 * over at most one block per CU.  A block finds the layer of a tile by a
 * search of plan[].tile0 (wave-uniform loads) and runs the row-table fold's
 * own tile body over xi + l*N with the layer's column count and output base,
 * so layer l of `out` (plan[l].cols elements at plan[l].offset) holds, bit for
 * bit, what fa_fedavg_*_ptrs gives for that layer alone: strict client order,
 * acc = t_0, separate multiply and add, the dtype's own divide, subnormals
 * kept, final stores non-temporal.  A layer with aligned == 0 (some row off
 * 16-B alignment) is folded one column per lane in the same launch.  Factors
 * are [device] arrays in the dtype's own convention (float32 for fp32 and
 * bf16 rows; binary16 bit patterns, the divisor too, for float16; double for
 * float64); bf16 takes the optional out_f32 / out_bf16 pair, at least one.
 * Every out is one flat array of the plan's `elems` elements, 16-B aligned;
 * the elements between a layer's end and the next offset are not written.
 * No allocation, no synchronisation.  Checked before any launch: negative
 * L / N / tiles, units outside {1, 2, 4}, a NULL xi / plan / a / out with
 * tiles > 0, an out off 16-B alignment -> FA_ERR_ARG; N == 0 ->
 * FA_ERR_NO_CLIENTS.  L == 0 or tiles == 0 launches nothing.  The plan and
 * the table live in device memory: the library cannot check them against
 * tiles and units, nor see an alias (no output may overlap a row).  Not
 * covered: a tuner kind (one fixed geometry: 8 rows ahead, units by
 * fa_layers_plan's rule), help for stream capture, the sharded step, several
 * GPUs.  Integer layers: fa_fedavg_i32_layers / fa_fedavg_i64_layers, below. */
typedef struct fa_layer_plan {
    int64_t cols;    /* columns of the layer                                  */
    int64_t offset;  /* its first element in the flat output (multiple of 64) */
    int64_t tile0;   /* its first tile (prefix sum of the layers' tiles)      */
    int64_t aligned; /* != 0: every row of the layer is 16-B aligned          */
} fa_layer_plan;
/* The host planner (touches no GPU).  cols[l], aligned[l]: the layers;
 * unit_lg: the columns of a 16-byte unit as a power of two (2 fp32, 3 bf16 /
 * float16, 1 float64); cus: the compute units the launch will have; units:
 * 1, 2 or 4 units per lane, or 0 for the rule -- the most of 4, 2, 1 whose
 * balanced grid over the model's total tiles still covers 7/8 of the CUs,
 * else 1.  Writes plan[0..L), *tiles (= tile0 of an L-th layer), *elems (the
 * flat output's length) and *units_out.  An aligned layer has
 * ceil(ceil(cols / unit) / (256 * units)) tiles, any other ceil(cols / 256). */
int fa_layers_plan(const int64_t* cols, const int32_t* aligned, int64_t L, int unit_lg, int64_t cus, int units,
                   fa_layer_plan* plan, int64_t* tiles, int64_t* elems, int* units_out);
int fa_fedavg_f32_layers(const float* const* xi, const fa_layer_plan* plan, int64_t L, int64_t N, int64_t tiles,
                         int units, const float* a, const float* s, float divisor, float* out, void* stream);
int fa_fedavg_bf16_layers(const uint16_t* const* xi, const fa_layer_plan* plan, int64_t L, int64_t N, int64_t tiles,
                          int units, const float* a, const float* s, float divisor, float* out_f32,
                          uint16_t* out_bf16, void* stream);
int fa_fedavg_f16_layers(const uint16_t* const* xi, const fa_layer_plan* plan, int64_t L, int64_t N, int64_t tiles,
                         int units, const uint16_t* a, const uint16_t* s, uint16_t divisor, uint16_t* out,
                         void* stream);
int fa_fedavg_f64_layers(const double* const* xi, const fa_layer_plan* plan, int64_t L, int64_t N, int64_t tiles,
                         int units, const double* a, const double* s, double divisor, double* out, void* stream);

/* Integer updates: numpy keeps `layer * n` and the np.add fold in the integer
 * dtype (wrapping) and true-divides into float64 (fed_avg_aggregator.py:33,39).
 * a = integer cardinalities [device, int64]; out float64. */
int fa_fedavg_i32(const int32_t* X, int64_t N, int64_t P, int64_t ldx,
                  const int64_t* a, double divisor, double* out, void* stream);
int fa_fedavg_i64(const int64_t* X, int64_t N, int64_t P, int64_t ldx,
                  const int64_t* a, double divisor, double* out, void* stream);

/* ---- integer layers where the clients' tensors lie (new symbols, ABI still 7)
 * A model with BatchNorm carries one int64 counter per BatchNorm layer next to
 * its float weights; these fold such layers through a row table, with no
 * stacking copy, in numpy's literal arithmetic (fed_avg_aggregator.py:33,39;
 * with scores stall_aware_aggregation.py:42-67).  T is the rows' dtype, UT its
 * unsigned twin, a[i] the cardinalities [device, int64], s[i] [device, double]:
 *   p_i = (T)((UT)x * (UT)(T)a[i])            wrapping, as `layer * n`
 *   s == NULL (FedAvg):   acc = p_0, acc = wrap(acc + p_i) in T;
 *                         out = (double)acc / divisor      -- what fa_fedavg_i32 /
 *                         fa_fedavg_i64 compute over the same rows stacked
 *   s != NULL (stall-aware): t_i = (double)p_i * s[i] -- numpy types `* s` in
 *                         float64; the conversion rounds to nearest even beyond
 *                         2^53, as numpy's cast -- acc = t_0, acc = acc + t_i in
 *                         strict client order, multiply and add separate;
 *                         out = acc / divisor
 * The divide is the float64 folds' IEEE divide (a subnormal quotient on a tie
 * rounds to even).  out is float64.
 *   fa_fedavg_i32_ptrs / _i64_ptrs: one layer, xi a [device] array of N
 *     [device] row pointers.  rows_aligned != 0 promises 16-B aligned rows and
 *     out (4 int32 / 2 int64 columns per 16-byte load, 8 rows ahead); with 0,
 *     rows at any offset of the element size and out at any 8-B offset, one
 *     column per lane.  The same bits either way.  Argument checks and status
 *     codes as fa_fedavg_f64_ptrs.  The layer's plan entry travels by value in
 *     the launch: no allocation, no copy, no synchronisation.
 *   fa_fedavg_i32_layers / _i64_layers: all L layers in one launch, xi / plan /
 *     tiles / units as the entries above, from fa_layers_plan with unit_lg 2
 *     (int32: four columns per 16 bytes) or 1 (int64).  The plan's offset and
 *     elems count OUTPUT elements, doubles: every layer starts at a multiple of
 *     64 doubles of the flat out, so a 16-B aligned out keeps every layer's
 *     stores aligned.  An int32 unit yields four doubles, stored as two 16-byte
 *     stores; final stores are non-temporal.  Layer l of out holds the bits of
 *     the _ptrs entry on that layer.  Argument checks and status codes as
 *     fa_fedavg_f64_layers.
 * Not covered: integer layers under float weights (the product is float64) and
 * int32 rows under int64 weights (the product is int64) -- the caller keeps
 * them off these entries; a tuner kind; help for stream capture; the sharded
 * step; several GPUs. */
int fa_fedavg_i32_ptrs(const int32_t* const* xi, int64_t N, int64_t P, const int64_t* a, const double* s,
                       double divisor, int rows_aligned, double* out, void* stream);
int fa_fedavg_i64_ptrs(const int64_t* const* xi, int64_t N, int64_t P, const int64_t* a, const double* s,
                       double divisor, int rows_aligned, double* out, void* stream);
int fa_fedavg_i32_layers(const int32_t* const* xi, const fa_layer_plan* plan, int64_t L, int64_t N, int64_t tiles,
                         int units, const int64_t* a, const double* s, double divisor, double* out, void* stream);
int fa_fedavg_i64_layers(const int64_t* const* xi, const fa_layer_plan* plan, int64_t L, int64_t N, int64_t tiles,
                         int units, const int64_t* a, const double* s, double divisor, double* out, void* stream);

/* ---- promoted folds from the narrow rows (new symbols, ABI still 7) ----------
 * numpy types `layer * num_examples` (fed_avg_aggregator.py:33; with scores
 * stall_aware_aggregation.py:52-66) by the operands: a numpy-scalar cardinality
 * (an np.int64 from len() of an array, an np.float32 weight) or a float
 * default_cardinality promotes the layer before the product, and the running
 * sum (fed_avg_aggregator.py:38-41) and the quotient stay in the promoted
 * dtype.  fa_fedavg_widen folds a stacked matrix of such rows without a widened
 * copy: each 16-byte unit of the rows' own dtype is converted in registers
 * right after its load, and the fold continues in the wide dtype's arithmetic.
 *   kind              rows      a, s      out      the bits of
 *   FA_WIDEN_F16_F32  binary16  float32   float32  fa_fedavg_f32 over the rows as float32
 *   FA_WIDEN_F16_F64  binary16  double    double   fa_fedavg_f64 over the rows as double
 *   FA_WIDEN_F32_F64  float32   double    double   fa_fedavg_f64 ...
 *   FA_WIDEN_I32_F64  int32     double    double   fa_fedavg_f64 over (double)x
 *   FA_WIDEN_I64_F64  int64     double    double   fa_fedavg_f64 over (double)x, which rounds
 *                                                  to nearest even beyond 2^53 as numpy's cast
 *   FA_WIDEN_I32_I64  int32     int64     double   fa_fedavg_i64 over the sign-extended rows:
 *                                                  wrapping product and sum, (double)acc / divisor
 * X is [N][ldx] in the rows' dtype, ldx in its elements; a and s are [device]
 * arrays in the kind's factor type, s NULL for FedAvg and always NULL for
 * FA_WIDEN_I32_I64 (a score makes that fold float64: FA_WIDEN_I32_F64); the
 * divisor is exact in a double for every kind (FA_WIDEN_F16_F32 is given a
 * value that is a float32).  Strict client order, acc = t_0, multiply and add
 * apart, the wide dtype's IEEE divide, subnormals kept, final stores
 * non-temporal.  One fixed geometry, no tuner kind: one block per tile of 256
 * lanes x `units` 16-byte source units, 8 rows of loads ahead of the ordered
 * adds (fa_widen_geometry reports it); X or out off 16-B alignment, or ldx not
 * a multiple of the unit's columns: one column per lane, 8 rows ahead, the same
 * bits.  Argument checks and status codes as fa_fedavg_f64; an unknown kind, or
 * s != NULL with FA_WIDEN_I32_I64 -> FA_ERR_ARG.  Not covered: row tables and
 * layer tables of promoted rows, folds numpy types term by term, the ingest
 * pipe, the sharded step. */
#define FA_WIDEN_F16_F32 0
#define FA_WIDEN_F16_F64 1
#define FA_WIDEN_F32_F64 2
#define FA_WIDEN_I32_F64 3
#define FA_WIDEN_I64_F64 4
#define FA_WIDEN_I32_I64 5
int fa_fedavg_widen(int kind, const void* X, int64_t N, int64_t P, int64_t ldx,
                    const void* a, const void* s, double divisor, void* out, void* stream);
/* [host] The geometry of a kind: the columns of a 16-byte source unit, the
 * units per lane of a tile, the rows of loads ahead.  Touches no GPU. */
int fa_widen_geometry(int kind, int* unit_cols, int* units, int* rows_ahead);

/* ---- host staging: page-locked documents and direct DMA ---------------------
 * A result store that keeps documents in page-locked memory lets the ingest
 * DMA each client's layers straight from the document into the device chunk,
 * with no host-side packing copy (fedlesscan_amd/ingest.py, store.py).
 *   fa_host_is_pinned: 1 if [p, p+n) lies inside ONE page-locked host
 *     allocation known to the HIP runtime (hipHostMalloc, hipHostRegister,
 *     torch pinned memory), else 0.  Never fails.
 *   fa_host_alloc / fa_host_free: hipHostMalloc / hipHostFree.
 *   fa_copy_h2d: hipMemcpyAsync host -> device of n bytes on stream. */
int fa_host_is_pinned(const void* p, int64_t n);
int fa_host_alloc(void** p, int64_t n);
int fa_host_free(void* p);
int fa_copy_h2d(void* dst, const void* src, int64_t n, void* stream);

/* ---- single-process multi-GPU ------------------------------------------------
 * The reference calls the strategy in-process, once per round
 * (aggregation.py:71-97).  The multi-GPU drop-in (fedlesscan_amd/multigpu.py)
 * folds one column bucket per GPU in that same process and reassembles the
 * model on one of them:
 *   fa_copy_peer: n bytes from src (on src_device) to dst (on dst_device),
 *     hipMemcpyPeerAsync over xGMI, enqueued on `stream` (normally the source
 *     GPU's stream that produced src, so it runs after that fold).  Peer
 *     access is enabled both ways the first time a pair is used.
 * Every compute entry above runs on the GPU that owns its stream, whatever
 * device the calling thread has current. */
int fa_copy_peer(void* dst, int dst_device, const void* src, int src_device, int64_t n, void* stream);

/* ---- native streaming ingest: host rows -> pinned slots -> DMA -> chunked fold --
 * The strategies' aggregate() (fed_avg_aggregator.py:57-92,
 * stall_aware_aggregation.py:82-117) decodes every client and then folds; here
 * each decoded row is handed over as it is decoded.  A process-wide pool of
 * copy workers packs rows into `slots` page-locked chunks of about chunk_bytes
 * (whole rows, pitch P rounded up to 64 floats); one issuer thread per pipe
 * sends each full chunk with one DMA on the pipe's copy stream and folds it on
 * the round's compute stream with fa_fold_f32, chunks in row order, the
 * accumulator carried across them: bit-identical to fa_fedavg_f32 over all
 * rows.  A chunk slot is refilled only after its fold has completed.  (These
 * entries are the float32 pipe; the float16 pipe's entries follow them.)
 *   fa_ingest_create:  allocate a pipe for models of P floats on `device`
 *   fa_ingest_begin:   start a round folding into acc [device, P] on `stream`;
 *                      expected_rows = the round's row count if known (0: not):
 *                      the first chunks hold 1, 2, 4, ... rows and, with the
 *                      count known, the last ones at most half of what is left,
 *                      so neither the start nor the tail waits for a full chunk
 *   fa_ingest_add:     one client row [host]: n pieces (srcs[i], sizes[i] bytes)
 *                      that concatenate to P floats, its factors a = fl32(n_i)
 *                      and s = fl32(score) when has_s (every row or none).  The
 *                      pieces must stay valid until fa_ingest_finish returns.
 *   fa_ingest_finish:  fold the last chunk and divide by `divisor`; returns when
 *                      every copy is done and every DMA and fold is enqueued
 *                      (the caller waits on `stream` for the result); after an
 *                      error it returns once no copy reads the pieces any more
 *   fa_ingest_destroy: wait for outstanding copies, free everything.
 * The pipe is reusable round after round (begin ... finish).  A begin after a
 * round that was abandoned (an add failed, or finish never came) drains that
 * round first (its queued chunks are not folded) and drops its partly filled
 * chunk, so none of its rows join the new round. */
typedef struct fa_ingest fa_ingest;
int fa_ingest_create(fa_ingest** pipe, int64_t P, int64_t chunk_bytes, int slots, int device);
int fa_ingest_rows_per_chunk(const fa_ingest* pipe);
int fa_ingest_begin(fa_ingest* pipe, float* acc, void* stream, int64_t expected_rows);
int fa_ingest_add(fa_ingest* pipe, const void* const* srcs, const int64_t* sizes, int64_t n, float a, float s,
                  int has_s);
int fa_ingest_finish(fa_ingest* pipe, float divisor);
int fa_ingest_destroy(fa_ingest* pipe);
/* The same pipe for float16 models (new symbols, ABI still 7): the reference's
 * aggregate() folds float16 results in binary16 (fed_avg_aggregator.py:57-92
 * over NEP 50 weak weights).  A pipe created with fa_ingest_create_f16 takes
 * rows of P halves (pitch P rounded up to 64 halves, chunk_bytes / (pitch * 2)
 * rows per chunk), the factors a, s and the divisor as binary16 bit patterns
 * (already rounded as numpy rounds them; inf stays inf), keeps its factor
 * block in halves ahead of the rows in the chunk's one DMA (padded so the rows
 * stay 256-B aligned) and folds into acc [device, P halves] with fa_fold_f16:
 * bit-identical to fa_fedavg_f16 over all rows.  Pieces of a row may hold any
 * whole number of halves.  Ramps, the halving tail, abandon and reuse, and the
 * error paths are those of the float32 pipe; fa_ingest_rows_per_chunk and
 * fa_ingest_destroy serve both kinds.  A float32 entry on a float16 pipe, or
 * the reverse, returns FA_ERR_ARG and leaves the pipe as it was. */
int fa_ingest_create_f16(fa_ingest** pipe, int64_t P, int64_t chunk_bytes, int slots, int device);
int fa_ingest_begin_f16(fa_ingest* pipe, uint16_t* acc, void* stream, int64_t expected_rows);
int fa_ingest_add_f16(fa_ingest* pipe, const void* const* srcs, const int64_t* sizes, int64_t n, uint16_t a,
                      uint16_t s, int has_s);
int fa_ingest_finish_f16(fa_ingest* pipe, uint16_t divisor);
/* The same pipe for float64 models (new symbols, ABI still 7): numpy's default
 * dtype, the reference's own aggregation fixture (test/test_aggregation.py:
 * 23-38) and what its aggregate() folds float64 results in
 * (fed_avg_aggregator.py:57-92, stall_aware_aggregation.py:82-117).  A pipe
 * created with fa_ingest_create_f64 takes rows of P doubles (pitch P rounded
 * up to 64 doubles, chunk_bytes / (pitch * 8) rows per chunk), the factors
 * a = fl64(n_i), s = fl64(score) and the divisor as doubles, keeps its factor
 * block in doubles ahead of the rows in the chunk's one DMA (padded to 256 B)
 * and folds into acc [device, P doubles] with fa_fold_f64: bit-identical to
 * fa_fedavg_f64 over all rows.  Pieces of a row are copied bytewise and may
 * start at any byte offset (views into NPZ blobs).  Ramps, the halving tail,
 * abandon and reuse, and the error paths are those of the float32 pipe; an
 * entry of one kind on a pipe of another returns FA_ERR_ARG and leaves the
 * pipe as it was. */
int fa_ingest_create_f64(fa_ingest** pipe, int64_t P, int64_t chunk_bytes, int slots, int device);
int fa_ingest_begin_f64(fa_ingest* pipe, double* acc, void* stream, int64_t expected_rows);
int fa_ingest_add_f64(fa_ingest* pipe, const void* const* srcs, const int64_t* sizes, int64_t n, double a,
                      double s, int has_s);
int fa_ingest_finish_f64(fa_ingest* pipe, double divisor);

/* ---- host-side ingest (no GPU): NPZ wire format -> pinned staging ----------
 * Client blobs are uncompressed NPZ archives (NpzWeightsSerializer,
 * serialization.py:280-306, written by the client, client.py:186-199). */
enum fa_dtype { FA_DT_F32 = 1, FA_DT_F64 = 2, FA_DT_I32 = 3, FA_DT_I64 = 4, FA_DT_F16 = 5,
                FA_DT_U8 = 6, FA_DT_I8 = 7, FA_DT_BOOL = 8 };
/* [host] Index the .npy members of an NPZ blob in archive order (= the order
 * of list(np.load(f).values()), serialization.py:304-306): payload byte offset,
 * element count, fa_dtype, ndim and shape (8 slots per layer).  Returns the
 * number of layers, or -1 when the blob must go through np.load instead
 * (compressed member, Fortran order, big-endian/object dtype, malformed, or
 * more than max_layers members).  All arrays are [host] with max_layers slots. */
int fa_npz_index(const uint8_t* blob, int64_t len, int64_t* offsets, int64_t* counts, int32_t* dtypes,
                 int32_t* ndims, int64_t* shapes, int max_layers);
/* [host] Copy n byte ranges: srcs[i] (sizes[i] bytes) -> dst + dst_offsets[i],
 * split by bytes over up to nthreads threads (0 = hardware concurrency).  The
 * pinned-staging packer of the ingest pipeline (fedlesscan_amd/ingest.py). */
int fa_pack(void* dst, const int64_t* dst_offsets, const void* const* srcs, const int64_t* sizes, int64_t n,
            int nthreads);
/* [host] zlib-compatible CRC-32 of data[0..n) continuing crc_in (0 to
 * start), split over up to nthreads threads (0 = hardware concurrency);
 * *crc_out = zlib.crc32(data, crc_in).  The member checksum of the NPZ writer
 * (fedlesscan_amd/npz.py write_npz: the saved round+1 model, aggregation.py
 * :139-147 -> NpzWeightsSerializer.serialize, serialization.py:290-296). */
int fa_crc32(const void* data, int64_t n, uint32_t crc_in, int nthreads, uint32_t* crc_out);

/* ---- host-side ingest (no GPU): the persisted BSON document -----------------
 * The reference stores each ClientResult as bson.encode(result.dict()) in
 * GridFS (client_daos.py:73) and reads it back with
 * ClientResult.parse_obj(bson.decode(file.read())) (client_daos.py:142), a
 * decode that copies the NPZ blob.  fa_bson_elements replaces the walk inside
 * bson.decode for one document level: for the document starting at
 * buf[doc_off] it reports, per element in order, the type byte, the name
 * (offset, length without NUL) and the value (offset, length):
 *   string/code/symbol -> the UTF-8 bytes without NUL; binary -> the payload
 *   (subtype in subtypes[], old subtype 2 unwrapped); document/array -> the
 *   embedded document itself (walk it with doc_off = its offset); fixed-size
 *   scalars -> their 1/4/8/12/16 bytes; null/undefined/min/max key -> length 0.
 * Offsets are relative to buf.  Returns the element count (only the first
 * max_elems are written; any output array may be NULL), or a negative
 * FA_BSON_* code.  Every length is bounds-checked against the enclosing
 * document. */
enum fa_bson_status { FA_BSON_MALFORMED = -1, FA_BSON_UNSUPPORTED = -2 };
int64_t fa_bson_elements(const uint8_t* buf, int64_t buf_len, int64_t doc_off, uint8_t* types,
                         int64_t* name_offs, int32_t* name_lens, int64_t* val_offs, int64_t* val_lens,
                         uint8_t* subtypes, int64_t max_elems);
/* [host] The whole tree of the document at buf[doc_off] in one call, in
 * pre-order: every element, then (for a document or array) its subtree.
 * parents[k] is the index of element k's enclosing document/array element, or
 * -1 at the top level; the other arrays as fa_bson_elements.  Nesting deeper
 * than 100 levels is FA_BSON_MALFORMED.  Returns the total element count. */
int64_t fa_bson_walk(const uint8_t* buf, int64_t buf_len, int64_t doc_off, uint8_t* types, int32_t* parents,
                     int64_t* name_offs, int32_t* name_lens, int64_t* val_offs, int64_t* val_lens,
                     uint8_t* subtypes, int64_t max_elems);

#ifdef __cplusplus
}
#endif
#endif /* FEDAVG_HIP_H */
