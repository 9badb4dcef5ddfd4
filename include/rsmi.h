/*
 * rsmi.h -- C-ABI of the MI355X Reed-Solomon engine (librsmi.so).
 *
 * This is the drop-in seam under filedag-storage's Dag Node: every entry point replaces
 * one call that dag/node/dagnode makes into github.com/klauspost/reedsolomon v1.11.0
 * (go.mod:31).  Plain pointers and sizes only -- no Go, torch or HIP types -- so a cgo
 * file binds it directly.  All functions are thread-safe; one context
 * may be shared by every goroutine of a DagNode (node.go:358 Put, :220 Get, the repair
 * worker at :159 and data_recovery.go:16 RepairDataNode all run concurrently).
 *
 * Buffer ownership: the caller owns every buffer; the library never retains a caller
 * pointer after a call returns (cgo pointer rules).  The *_dev entry points take device
 * pointers and a hipStream_t passed as void*; they are stream-ordered and do not sync.
 * Two exceptions: the first call of a context that needs a device table (CRC-16, CRC-32,
 * locate) or a plan (the encode's, one per erasure pattern) allocates it and fills it with a
 * blocking copy, which waits for work queued on the NULL stream and on every stream created without
 * hipStreamNonBlocking (the caller's own too, if it is such a stream); and per-stream scratch
 * that has to grow or start over waits for that stream once, as the entry points below state.
 *
 * Status codes map 1:1 onto the upstream sentinels (erasure.go:19,23 return two of them
 * directly; the rest surface through Split/Encode/Reconstruct at erasure.go:55,60,82,88).
 * There is no CPU fallback: a device failure is RSMI_ERR_DEVICE / RSMI_ERR_NO_DEVICE.
 */
#ifndef RSMI_H
#define RSMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: rsmi_set_option lost the keys of kernel variants measured slower than the defaults (they
 * return RSMI_ERR_INVALID_ARG); device groups, NUMA placement, the key slot hash and
 * rsmi_reconstruct_batch_host_verify were added; "crc16_fused_fold" is new.
 * 3: no C++ exception crosses the boundary: every status-returning entry point that can allocate
 * on the host returns RSMI_ERR_HOST instead (new status).
 * 4: coalesced calls run on up to "coalesce_lanes" batches at once (new option, default 2);
 * rsmi_warm is new; the device-resident CRC entry points may run concurrently on different streams
 * of one context; rsmi_last_kernel returns a per-thread copy.
 * 5: the per-thread wait hook (rsmi_set_wait_hook, rsmi_run_wait_hook).  The Encoder.Verify entry
 * points (rsmi_verify, rsmi_verify_batch_host, rsmi_verify_batch_dev) joined version 5: additive;
 * so did the locate entry points (rsmi_locate, rsmi_locate_batch_host, rsmi_locate_batch_dev,
 * rsmi_locate_matrix), the heal entry points (rsmi_heal, rsmi_heal_batch_host,
 * rsmi_heal_batch_dev), the mixed-batch reconstruct (rsmi_reconstruct_mixed_batch_dev,
 * rsmi_reconstruct_mixed_batch_host, rsmi_reconstruct_mixed_classify), the pair locate
 * (rsmi_locate_pair, rsmi_locate_pair_batch_host, rsmi_locate_pair_batch_dev,
 * rsmi_locate_pair_checks), the pair heal (rsmi_heal_pair, rsmi_heal_pair_batch_host,
 * rsmi_heal_pair_batch_dev, rsmi_heal_pair_matrix), the scrub (rsmi_scrub, rsmi_scrub_batch_host,
 * rsmi_scrub_batch_dev) and the checksums of named rows (rsmi_crc_named_rows_dev,
 * rsmi_reconstruct_mixed_batch_dev_crcs, rsmi_reconstruct_mixed_batch_host_crcs) and the mixed
 * reconstruct that checksums what it reads and writes (rsmi_reconstruct_mixed_batch_dev_verify,
 * rsmi_reconstruct_mixed_batch_host_verify) and the ragged encode (rsmi_encode_ragged_batch_dev,
 * rsmi_encode_ragged_batch_host, rsmi_encode_ragged_classify). */
#define RSMI_ABI_VERSION 5

typedef struct rsmi_ctx rsmi_ctx;

enum rsmi_status {
    RSMI_OK = 0,
    RSMI_ERR_SHORT_DATA = 1,     /* reedsolomon.ErrShortData    (Split of 0 bytes)          */
    RSMI_ERR_TOO_FEW_SHARDS = 2, /* reedsolomon.ErrTooFewShards (< k shards present)        */
    RSMI_ERR_SHARD_NO_DATA = 3,  /* reedsolomon.ErrShardNoData  (every shard empty)         */
    RSMI_ERR_SHARD_SIZE = 4,     /* reedsolomon.ErrShardSize    (unequal non-empty shards)  */
    RSMI_ERR_INV_SHARD_NUM = 5,  /* reedsolomon.ErrInvShardNum  (k<=0 || m<=0), erasure.go:19 */
    RSMI_ERR_MAX_SHARD_NUM = 6,  /* reedsolomon.ErrMaxShardNum  (k+m>256),     erasure.go:23 */
    RSMI_ERR_SINGULAR = 7,       /* matrix not invertible (cannot happen for valid patterns) */
    RSMI_ERR_INVALID_ARG = 8,    /* NULL pointer, stride smaller than a shard, ...          */
    RSMI_ERR_DEVICE = 100,       /* a HIP call failed                                       */
    RSMI_ERR_NO_DEVICE = 101,    /* no usable gfx950 device / kernels not loadable          */
    RSMI_ERR_HOST = 102          /* host resources exhausted (memory, threads): a C++
                                  * exception caught at the boundary, never propagated     */
};

/* ------------------------------------------------------------------ lifecycle */

/* Replaces reedsolomon.New(k, m, WithAutoGoroutines(S)) inside NewErasure
 * (dag/node/dagnode/erasure.go:16-47).  Validates like erasure.go:18-24, builds and caches
 * the n x k systematic matrix.  Device resources are created lazily on first compute call,
 * so opening a context works (and reports argument errors) on a host without a GPU. */
int rsmi_open(int k, int m, int device, rsmi_ctx** out);
void rsmi_close(rsmi_ctx* ctx);

/* Bring up the context's device resources before the first real call (a Dag Node does this when
 * it starts): streams, the encode plan, the CRC tables and every coalescing lane (one tiny fused
 * encode + CRC-16 each), so the first concurrent callers do not pay for them. */
int rsmi_warm(rsmi_ctx* ctx);

int rsmi_device_count(void);
const char* rsmi_status_string(int status);
int rsmi_abi_version(void);

/* ------------------------------------------------------------------ host-only helpers */

/* Erasure.ShardSize (erasure.go:96-98) = ceilFrac(B, k) (utils.go:6-21). */
size_t rsmi_shard_size(size_t block_size, int k);

/* Device row pitch for shards of S bytes that the fast kernels stream best on MI355X:
 * the next power of two for shards up to 64 KiB (when it wastes at most half a shard) and
 * for exact powers of two, 11/8 S in 4 KiB granules for 96 KiB < S < 128 KiB (1 MiB RS(10,4)
 * blocks), otherwise S rounded up to 4 KiB (measured, DESIGN.md "Layout").  The
 * host-staged entry points use it internally. */
size_t rsmi_recommended_pitch(size_t S);

/* The cached (k+m) x k encode matrix, row-major. */
int rsmi_encode_matrix(const rsmi_ctx* ctx, uint8_t* out);

/* Upstream checkShards/shardSize: lens[i]==0 marks shard i missing.  nil_ok=0 is the
 * Encode check, nil_ok=1 the Reconstruct check.  *S_out receives the common size. */
int rsmi_check_shards(int n, const size_t* lens, int nil_ok, size_t* S_out);

/* The k x k data-decode matrix the reconstruct path uses for this erasure pattern
 * (inverse of the rows of the first k present shards, upstream reconstruct()); the k
 * survivor indices are written to used_rows.  present: n flags. */
int rsmi_decode_matrix(const rsmi_ctx* ctx, const uint8_t* present, uint8_t* out, int* used_rows);

/* ------------------------------------------------------------------ one block, host memory */

/* Erasure.EncodeData (erasure.go:51-65): Split + Encode of one raw block of B bytes into
 * (k+m)*S contiguous bytes, S = rsmi_shard_size(B, k); data rows zero-padded like Split.
 * B == 0 -> RSMI_ERR_SHORT_DATA (the Go wrapper short-circuits it before calling). */
int rsmi_encode_block(rsmi_ctx* ctx, const uint8_t* block, size_t B, uint8_t* shards_out);

/* Encoder.Encode on pre-split shards: data = k*S contiguous, parity = m*S contiguous. */
int rsmi_encode(rsmi_ctx* ctx, const uint8_t* data, uint8_t* parity, size_t S);

/* Encoder.ReconstructData (data_only=1, erasure.go:82) / Encoder.Reconstruct (data_only=0,
 * erasure.go:88) on n*S contiguous bytes.  present: n flags; missing rows are overwritten,
 * present rows are only read.  Nothing missing -> RSMI_OK without touching the device. */
int rsmi_reconstruct(rsmi_ctx* ctx, uint8_t* shards, size_t S, const uint8_t* present, int data_only);

/* ------------------------------------------------------------------ batches, host memory */

/* nblocks independent blocks: data block b at data + b*data_block_stride (k rows of S
 * bytes), parity block b at parity + b*parity_block_stride (m rows of S bytes).
 * Copies are overlapped with compute over several HIP streams; pass memory from
 * rsmi_host_alloc for full PCIe rate. */
int rsmi_encode_batch_host(rsmi_ctx* ctx, const uint8_t* data, size_t data_block_stride, uint8_t* parity,
                           size_t parity_block_stride, size_t S, size_t nblocks);

/* One erasure pattern for every block (RepairDataNode shape, data_recovery.go:16-112):
 * block b at shards + b*block_stride holds n rows of S bytes. */
int rsmi_reconstruct_batch_host(rsmi_ctx* ctx, uint8_t* shards, size_t block_stride, size_t S, size_t nblocks,
                                const uint8_t* present, int data_only);

/* Rebuild only the rows flagged in required[] (n flags; rows that are present are left
 * alone) -- RepairDataNode needs one row per key (data_recovery.go:88,102-106), not every
 * missing one.  Same layout and errors as rsmi_reconstruct_batch_host. */
int rsmi_reconstruct_rows_batch_host(rsmi_ctx* ctx, uint8_t* shards, size_t block_stride, size_t S, size_t nblocks,
                                     const uint8_t* present, const uint8_t* required);

/* Page-locked host memory: portable (mapped for every device, so device-group members read and
 * write one buffer in place) and placed by the calling thread's NUMA memory policy. */
void* rsmi_host_alloc(size_t bytes);
void rsmi_host_free(void* p);

/* ------------------------------------------------------------------ batches, device memory */

/* Device-resident encode.  Row c of data block b is at
 *   d_data + b*data_block_stride + c*data_shard_stride
 * and parity row j at d_parity + b*parity_block_stride + j*parity_shard_stride.
 * Fast path: every base/stride a multiple of 16 and each shard stride >= S rounded up to
 * 16 (the rows' padding bytes may be read, are never written).  Any other layout runs a
 * byte-granular kernel.  stream: hipStream_t (NULL = default stream). */
int rsmi_encode_batch_dev(rsmi_ctx* ctx, const uint8_t* d_data, size_t data_shard_stride,
                          size_t data_block_stride, uint8_t* d_parity, size_t parity_shard_stride,
                          size_t parity_block_stride, size_t S, size_t nblocks, void* stream);

/* Device-resident in-place reconstruct, one erasure pattern for all blocks.  Row i of
 * block b at d_shards + b*block_stride + i*shard_stride. */
int rsmi_reconstruct_batch_dev(rsmi_ctx* ctx, uint8_t* d_shards, size_t shard_stride, size_t block_stride,
                               size_t S, size_t nblocks, const uint8_t* present, int data_only, void* stream);

/* Device-resident form of rsmi_reconstruct_rows_batch_host. */
int rsmi_reconstruct_rows_batch_dev(rsmi_ctx* ctx, uint8_t* d_shards, size_t shard_stride, size_t block_stride,
                                    size_t S, size_t nblocks, const uint8_t* present, const uint8_t* required,
                                    void* stream);

/* ------------------------------------------------------------------ mixed batches: a pattern per block */

/* The reconstruct calls above take one erasure pattern for the whole batch, which fits a repair
 * after one datanode is lost.  Checksum failures, slow or failed fetches and half-finished repairs
 * give every block its own pattern; these calls rebuild such a batch in one go, with no sort of the
 * blocks by pattern and no call per pattern.
 *   Masks.  present and required hold nblocks x (k+m) bytes in HOST memory, block-major: byte
 *   b*(k+m) + i is the flag of row i of block b.  They are read before the call returns: the caller
 *   may free or overwrite them at once, also after the stream-ordered _dev call.  required == NULL:
 *   the rows to rebuild in a block are its missing data rows (data_only != 0) or all its missing
 *   rows (data_only == 0), as rsmi_reconstruct_batch_*.  required != NULL: per block the rule of
 *   rsmi_reconstruct_rows_batch_* (the missing rows that are flagged), data_only is ignored.
 *   What is written.  In every block whose status is RSMI_OK, bytes [0, S) of each wanted missing
 *   row are written, and they are the bytes rsmi_reconstruct_rows_batch_dev writes for that block
 *   alone under that block's masks: the survivors are the first k present rows, data rows come from
 *   the inverse of their sub-matrix, missing parity rows from M[i] x inverse.  Nothing else is
 *   written: no present row, no missing row that is not wanted, no byte at or past S of any row, no
 *   byte of a gap, no byte of a block that has nothing to rebuild, no byte of a block with fewer
 *   than k rows present.  The layout contract holds: padding may be read and is never written.
 *   Status.  status_out (host memory, nblocks int32, may be NULL) receives per block RSMI_OK or
 *   RSMI_ERR_TOO_FEW_SHARDS (a wanted row is missing and fewer than k rows are present; a block
 *   that has nothing to rebuild is RSMI_OK whatever it has present, as upstream).  With status_out
 *   given the call rebuilds the other blocks and returns RSMI_OK; with status_out == NULL a batch
 *   with such a block returns RSMI_ERR_TOO_FEW_SHARDS before any launch and writes nothing, the
 *   whole-batch behaviour of the calls above.  status_out is written only when the call returns
 *   RSMI_OK.
 *   Arguments.  The checks, their order and their statuses are those of rsmi_reconstruct_batch_dev
 *   / _host: a NULL ctx, shards or present -> RSMI_ERR_INVALID_ARG; S == 0 ->
 *   RSMI_ERR_SHARD_NO_DATA; a shard stride below S, or (host) a block stride below (k+m)*S ->
 *   RSMI_ERR_INVALID_ARG; nblocks == 0 -> RSMI_OK.  They come before any device access, as does the
 *   classing of the masks: a batch with nothing to rebuild returns RSMI_OK without a device, any
 *   other on a host without a GPU RSMI_ERR_NO_DEVICE, with nothing written.
 * The calls are joined to ABI version 5 (additive); none of them takes or clears the per-thread
 * wait hook. */

/* Device-resident, in place: row i of block b at d_shards + b*block_stride + i*shard_stride, fast
 * path alignment as rsmi_encode_batch_dev.  Stream-ordered, no sync: the blocks' classes travel to
 * per-stream scratch on the same stream (growing it, or starting it over once it is used up,
 * waits for that stream once). */
int rsmi_reconstruct_mixed_batch_dev(rsmi_ctx* ctx, uint8_t* d_shards, size_t shard_stride, size_t block_stride,
                                     size_t S, size_t nblocks, const uint8_t* present, const uint8_t* required,
                                     int data_only, int32_t* status_out, void* stream);

/* Host memory: block b at shards + b*block_stride holds k+m rows of S bytes.  Page-locked shards
 * (rsmi_host_alloc) are rebuilt where they lie; small pageable calls are staged by CPU copies;
 * larger ones are uploaded in chunks of whole blocks, and only the rebuilt rows come back. */
int rsmi_reconstruct_mixed_batch_host(rsmi_ctx* ctx, uint8_t* shards, size_t block_stride, size_t S, size_t nblocks,
                                      const uint8_t* present, const uint8_t* required, int data_only,
                                      int32_t* status_out);

/* rsmi_reconstruct_mixed_batch_dev (same arguments, results, statuses and writes) plus the raw
 * checksums of every row it rebuilt: d_raw16_out / d_raw32_out[b*(k+m) + r] = R / R32 of row r of
 * block b where the call wrote that row, 0 everywhere else -- rows that are present, rows that are
 * not wanted, blocks with RSMI_ERR_TOO_FEW_SHARDS -- as rsmi_reconstruct_rows_batch_host_crcs defines
 * them (device memory, nblocks*(k+m) words each, either may be NULL, not both: RSMI_ERR_INVALID_ARG
 * with the NULL checks).  The outputs are zeroed on the stream and the rows pass over the rebuilt
 * rows (rsmi_crc_named_rows_dev's kernels) follows the rebuild on it; the rows it visits ride in
 * the same upload as the blocks' classes, so no copy and no wait is added.  A batch with nothing to
 * rebuild still zeroes the outputs on the stream: unlike the call above it then needs the device
 * (RSMI_ERR_NO_DEVICE without one).  When the call fails as a whole the outputs are unspecified. */
int rsmi_reconstruct_mixed_batch_dev_crcs(rsmi_ctx* ctx, uint8_t* d_shards, size_t shard_stride, size_t block_stride,
                                          size_t S, size_t nblocks, const uint8_t* present, const uint8_t* required,
                                          int data_only, int32_t* status_out, uint32_t* d_raw16_out,
                                          uint32_t* d_raw32_out, void* stream);

/* rsmi_reconstruct_mixed_batch_host plus the same checksums in host memory (raw16_out / raw32_out,
 * nblocks*(k+m) words each, either may be NULL, not both), on each of its three paths from the GPU
 * where the rows were rebuilt.  A batch with nothing to rebuild zeroes them and returns RSMI_OK
 * without a device.  RepairDataNode's Puts of rows rebuilt from a mixed flush carry sender
 * checksums as rsmi_reconstruct_rows_batch_host_crcs gives them for a uniform one. */
int rsmi_reconstruct_mixed_batch_host_crcs(rsmi_ctx* ctx, uint8_t* shards, size_t block_stride, size_t S,
                                           size_t nblocks, const uint8_t* present, const uint8_t* required,
                                           int data_only, int32_t* status_out, uint32_t* raw16_out,
                                           uint32_t* raw32_out);

/* rsmi_reconstruct_mixed_batch_dev (same arguments, checks in the same order with the same statuses,
 * masks' lifetime, status_out and bytes written into the shards, the whole-batch
 * RSMI_ERR_TOO_FEW_SHARDS before any launch when status_out == NULL included) plus R, the datanode's
 * raw CRC-16, of every row the call touches, so a caller rebuilds no shard from a bad survivor
 * unnoticed: the mixed form of rsmi_reconstruct_batch_host_verify.  d_raw16_rows (device memory,
 * nblocks*(k+m) words, required: NULL -> RSMI_ERR_INVALID_ARG with the NULL checks) is zeroed on the
 * stream first.  For a block with status RSMI_OK that has something to rebuild,
 * d_raw16_rows[b*(k+m) + r] = R over bytes [0, S) of row r where the call touched that row:
 *   rows it read     the first k present rows (rsmi_decode_matrix's used_rows for the block's mask),
 *   rows it wrote    the wanted missing rows,
 * and 0 for every other row of the block (present rows beyond the first k, missing rows that are
 * not wanted).  Every row of a block the call does not touch -- one with nothing to rebuild, one with
 * RSMI_ERR_TOO_FEW_SHARDS -- gets 0; a caller that wants those rows checked runs rsmi_crc16_rows_dev
 * (host memory: rsmi_crc_rows_host) on them.  Each value is what rsmi_crc16_rows_dev gives for the
 * row as it lies in memory after the call (a damaged survivor's R is that of its stored bytes), and
 * rsmi_crc16_entry finishes it.  Padding may be read; it is never written and never reaches a
 * checksum.  Where the shape has a kernel for it (k in {1,2,3,4,5,6,8,10,12,16}, at most 4 rows to
 * rebuild in a block, rows 16-byte aligned or S >= 16) the checksums come from the one read of the
 * survivors that rebuilds the rows; other blocks are rebuilt as above and their rows then read by
 * rsmi_crc_named_rows_dev's kernels.  Stream-ordered, no sync (per-stream scratch grows as above);
 * like _dev_crcs a batch with nothing to rebuild still needs the device to zero the output
 * (RSMI_ERR_NO_DEVICE without one).  When the call fails as a whole the output is unspecified. */
int rsmi_reconstruct_mixed_batch_dev_verify(rsmi_ctx* ctx, uint8_t* d_shards, size_t shard_stride,
                                            size_t block_stride, size_t S, size_t nblocks, const uint8_t* present,
                                            const uint8_t* required, int data_only, int32_t* status_out,
                                            uint32_t* d_raw16_rows, void* stream);

/* rsmi_reconstruct_mixed_batch_host plus the same checksums in host memory (raw16_rows,
 * nblocks*(k+m) words, required), on each of its three paths.  On page-locked shards, which are
 * coded where they lie, every survivor crosses PCIe once for both the rebuild and its checksum.  A
 * batch with nothing to rebuild zeroes raw16_rows and returns RSMI_OK without a device; any other on
 * a host without a GPU returns RSMI_ERR_NO_DEVICE.  Only wanted rows are written back. */
int rsmi_reconstruct_mixed_batch_host_verify(rsmi_ctx* ctx, uint8_t* shards, size_t block_stride, size_t S,
                                             size_t nblocks, const uint8_t* present, const uint8_t* required,
                                             int data_only, int32_t* status_out, uint32_t* raw16_rows);

/* Host-only, works without a GPU, like rsmi_decode_matrix: what the two calls above will do with
 * these masks.  Every output may be NULL.  status_out[b]: as above.  rows_out[b]: the rows the call
 * writes in block b, 0..m (0 for a block with too few rows present).  pattern_out[b]: the index of
 * the block's distinct (present, want) pair, numbered by first appearance, where present is taken
 * as 0 / 1 per row and want is "this row is missing and to be rebuilt"; blocks with equal indices
 * share one decode matrix and one set of kernel tables.  *npatterns_out: the number of pairs. */
int rsmi_reconstruct_mixed_classify(const rsmi_ctx* ctx, size_t nblocks, const uint8_t* present,
                                    const uint8_t* required, int data_only, int32_t* status_out, uint8_t* rows_out,
                                    uint32_t* pattern_out, size_t* npatterns_out);

/* ------------------------------------------------------------------ ragged batches: a size per block */

/* The encode calls above take one S for the whole batch.  A Dag Node's blocks do not share a size:
 * a file is a run of full chunks, one tail chunk of any length and a few small link nodes.  These
 * calls encode such a batch in one go, with no sort of the blocks by size and no call per size.
 *   Blocks.  blocks holds nblocks descriptors in HOST memory.  They are read before the call
 *   returns: the caller may free or overwrite them at once, also after the stream-ordered _dev call.
 *   Data row c of a block is at data_base + data_off + c*data_shard_stride, parity row j at
 *   parity_base + parity_off + j*parity_shard_stride; the two halves are independent.  A block's
 *   parity rows must not overlap any row of any block; data rows may be shared between blocks.
 *   What is written.  For every block, bytes [0, S) of its m parity rows, and they are the bytes
 *   rsmi_encode_batch_dev writes for that block alone (nblocks = 1) at the same addresses and
 *   strides.  Nothing else is written: no data row, no byte at or past S of any row, no byte of a
 *   gap.  The layout contract holds: padding may be read and is never written.
 *   Arguments.  All checks come before any device access: a NULL ctx, base or blocks ->
 *   RSMI_ERR_INVALID_ARG; nblocks == 0 -> RSMI_OK; then the blocks in index order, the first bad
 *   block deciding the status, per block in the order of rsmi_encode_batch_dev: S == 0 ->
 *   RSMI_ERR_SHARD_NO_DATA, then a shard stride below S -> RSMI_ERR_INVALID_ARG.  Nothing is
 *   written when a call fails on its arguments; on a host without a GPU a call that passes them
 *   returns RSMI_ERR_NO_DEVICE.
 * The calls are joined to ABI version 5 (additive); none of them takes or clears the per-thread
 * wait hook. */
typedef struct rsmi_ragged_block {
    uint64_t S;                   /* this block's shard size, > 0 */
    uint64_t data_off;            /* data row c   at d_data   + data_off   + c * data_shard_stride   */
    uint64_t data_shard_stride;
    uint64_t parity_off;          /* parity row j at d_parity + parity_off + j * parity_shard_stride */
    uint64_t parity_shard_stride;
} rsmi_ragged_block;

/* What the device call does with a block (rsmi_encode_ragged_classify). */
#define RSMI_RAGGED_ALIGNED 0  /* rows 16-byte aligned, strides multiples of 16 and >= S rounded up to 16 */
#define RSMI_RAGGED_UA 1       /* any other rows of at least 16 bytes: the unaligned-window kernels    */
#define RSMI_RAGGED_FALLBACK 2 /* S < 16 on unaligned rows, k not in {1..6,8,10,12,16}, S >= 2^31:
                                * rsmi_encode_batch_dev's launch for that block alone               */

/* Device-resident.  Stream-ordered, no sync: the blocks' descriptors travel to per-stream scratch
 * on the same stream (growing it, or starting it over once it is used up, waits for that stream
 * once).  One launch per class of blocks (aligned, unaligned-window) and tile of the encode plan
 * (m > 4: several), whatever the number of distinct sizes; fallback blocks are launched one by one
 * behind them. */
int rsmi_encode_ragged_batch_dev(rsmi_ctx* ctx, const uint8_t* d_data, uint8_t* d_parity,
                                 const rsmi_ragged_block* blocks, size_t nblocks, void* stream);

/* The same descriptors over host bases; the rows are already Split, as for rsmi_encode_batch_host.
 * With both halves page-locked (rsmi_host_alloc) the rows are coded where they lie; otherwise they
 * are staged through page-locked memory by CPU copies, in chunks of whole blocks, and only bytes
 * [0, S) of the parity rows are copied back. */
int rsmi_encode_ragged_batch_host(rsmi_ctx* ctx, const uint8_t* data, uint8_t* parity,
                                  const rsmi_ragged_block* blocks, size_t nblocks);

/* Host-only, works without a GPU: what rsmi_encode_ragged_batch_dev will do with each block of these
 * descriptors over these bases.  class_out[b] (may be NULL): RSMI_RAGGED_*.  tiles_out[b] (may be
 * NULL): the block's 1 KiB-per-row tiles per tile of the encode plan, 0 for a fallback block.  The
 * base pointers are used for their alignment only and are never dereferenced (they may be NULL).
 * The blocks pass the calls' checks first, with their statuses. */
int rsmi_encode_ragged_classify(const rsmi_ctx* ctx, const void* data_base, const void* parity_base,
                                const rsmi_ragged_block* blocks, size_t nblocks, uint8_t* class_out,
                                uint64_t* tiles_out);

/* ------------------------------------------------------------------ Encoder.Verify */

/* Do the k+m shards of a block belong together: is every parity row what Encode would produce
 * from the data rows?  The Dag Node never calls Verify; it is offered for scrubs of stored
 * stripes and for confirming a repair or a migration before the old copy is dropped.  A shard
 * checksum says a shard is the bytes that were stored; only this check says it is the right
 * shard for the stripe (not stale, swapped between keys, or rebuilt from a bad survivor).  The
 * check reads k+m rows and writes only flags; bytes outside a row (padding) never count.  None of
 * these calls takes or clears the per-thread wait hook. */

/* Encoder.Verify, device-resident: layout as rsmi_encode_batch_dev; nothing is written but
 * d_bad_out[b*m + j] (device memory, nblocks*m words, zeroed first on the stream), non-zero iff
 * parity row j of block b differs from the encode of its data rows.  Stream-ordered, no sync. */
int rsmi_verify_batch_dev(rsmi_ctx* ctx, const uint8_t* d_data, size_t data_shard_stride, size_t data_block_stride,
                          const uint8_t* d_parity, size_t parity_shard_stride, size_t parity_block_stride,
                          size_t S, size_t nblocks, uint32_t* d_bad_out, void* stream);

/* Host memory, layout as rsmi_encode_batch_host; bad_out[b*m + j] in host memory.  Page-locked
 * data and parity (rsmi_host_alloc) are read in place over PCIe by one kernel; small pageable
 * calls are staged by CPU copies; larger ones are uploaded in chunks that overlap the check. */
int rsmi_verify_batch_host(rsmi_ctx* ctx, const uint8_t* data, size_t data_block_stride, const uint8_t* parity,
                           size_t parity_block_stride, size_t S, size_t nblocks, uint32_t* bad_out);

/* Encoder.Verify of one block: n*S contiguous bytes; *ok_out = 1 iff every parity row matches. */
int rsmi_verify(rsmi_ctx* ctx, const uint8_t* shards, size_t S, int* ok_out);

/* ------------------------------------------------------------------ scrub: Verify and every shard's CRC-16 */

/* A scrub of stored stripes asks two questions of every shard it reads: is it the bytes that were
 * stored (the datanode's CRC-16 of the entry, server.go:70), and do the k+m shards belong together
 * (Verify)?  These calls answer both from one read of the k+m rows: Verify's flags, and R(shard)
 * of every data and parity row as stored, damaged or not, which rsmi_crc16_entry finishes on the
 * host (see "datanode CRC-16" below).  The read-side twin of rsmi_encode_batch_dev_crc.  Shapes
 * without a one-pass kernel (m > 4, a k without one, unaligned rows shorter than 16 bytes) run
 * Verify and the CRC-16 rows pass one after the other, with the same results.  Nothing but the two
 * outputs is written; bytes outside a row (padding) reach neither.  None of these calls takes or
 * clears the per-thread wait hook. */

/* Device-resident: layout, argument checks and fast-path alignment as rsmi_verify_batch_dev.
 * d_bad_out[b*m + j] (nblocks*m words) is exactly rsmi_verify_batch_dev's flags, and
 * d_raw_out[b*(k+m) + r] (nblocks*(k+m) words, data rows first) exactly what rsmi_crc16_rows_dev
 * writes for that row: R(shard) over bytes [0, S).  Both are required, both device memory.
 * Stream-ordered, no sync (the stream's scratch grows behind one wait for that stream). */
int rsmi_scrub_batch_dev(rsmi_ctx* ctx, const uint8_t* d_data, size_t data_shard_stride, size_t data_block_stride,
                         const uint8_t* d_parity, size_t parity_shard_stride, size_t parity_block_stride,
                         size_t S, size_t nblocks, uint32_t* d_bad_out, uint32_t* d_raw_out, void* stream);

/* Host memory, layout and the three paths of rsmi_verify_batch_host (page-locked rows are read in
 * place, once); bad_out[b*m + j] and raw16_out[b*(k+m) + r] in host memory, both required. */
int rsmi_scrub_batch_host(rsmi_ctx* ctx, const uint8_t* data, size_t data_block_stride, const uint8_t* parity,
                          size_t parity_block_stride, size_t S, size_t nblocks, uint32_t* bad_out,
                          uint32_t* raw16_out);

/* One block of n*S contiguous bytes: *ok_out = 1 iff every parity row matches, raw_out[0..k+m) =
 * R(shard). */
int rsmi_scrub(rsmi_ctx* ctx, const uint8_t* shards, size_t S, int* ok_out, uint32_t* raw_out);

/* ------------------------------------------------------------------ locate: which shard is wrong */

/* Verify says that a stripe's shards do not belong together; locate names the shard that breaks
 * it, which no shard checksum can (a stale or swapped shard passes its own CRC).  A stripe is
 * clean when every parity row equals the encode of the data rows over bytes [0, S); padding never
 * counts.  Shard x (0..k+m-1) explains a dirty stripe when replacing row x by its reconstruction
 * from the other rows yields a clean stripe.  The verdict of a block is
 *   RSMI_LOCATE_CLEAN    the stripe is clean;
 *   x in [0, k+m)        the stripe is dirty and shard x is the only shard that explains it;
 *   RSMI_LOCATE_UNKNOWN  the stripe is dirty and no shard, or more than one, explains it.
 * What the code's distance (m + 1) gives -- a property of the code, not of the implementation:
 *   m = 1        every shard explains any damage, so a dirty stripe is always UNKNOWN;
 *   m >= 2       a single damaged shard, however many of its bytes, is always named;
 *   m >= 2t      t >= 2 damaged shards are always UNKNOWN (rsmi_locate_pair below names two);
 *   beyond that  the damage can imitate a single other shard (its syndromes can be those of
 *                that shard alone); the verdict is then that shard: it is the unique explanation.
 * Every shard is taken as present (there are no missing-shard flags).  The calls are joined to ABI
 * version 5 (additive); none of them takes or clears the per-thread wait hook. */
#define RSMI_LOCATE_CLEAN (-1)
#define RSMI_LOCATE_UNKNOWN (-2)

/* Device-resident: layout, argument checks and fast-path alignment as rsmi_verify_batch_dev.  One
 * pass over the k+m rows yields d_culprit_out[b] (device memory, nblocks verdicts) and, when
 * d_bad_out is not NULL, d_bad_out[b*m + j], exactly rsmi_verify_batch_dev's flags.  Nothing else
 * is written.  Stream-ordered, no sync (scratch is kept per stream; growing it waits for that
 * stream once). */
int rsmi_locate_batch_dev(rsmi_ctx* ctx, const uint8_t* d_data, size_t data_shard_stride, size_t data_block_stride,
                          const uint8_t* d_parity, size_t parity_shard_stride, size_t parity_block_stride,
                          size_t S, size_t nblocks, int32_t* d_culprit_out, uint32_t* d_bad_out, void* stream);

/* Host memory, layout and the three paths of rsmi_verify_batch_host; culprit_out[b] and (when not
 * NULL) bad_out[b*m + j] in host memory. */
int rsmi_locate_batch_host(rsmi_ctx* ctx, const uint8_t* data, size_t data_block_stride, const uint8_t* parity,
                           size_t parity_block_stride, size_t S, size_t nblocks, int32_t* culprit_out,
                           uint32_t* bad_out);

/* One block of n*S contiguous bytes: *culprit_out receives its verdict. */
int rsmi_locate(rsmi_ctx* ctx, const uint8_t* shards, size_t S, int* culprit_out);

/* Host-only, works without a GPU: the m x k ratio matrix R[j][c] = M[k+j][c] / M[k][c] of the
 * encode matrix's parity rows (row 0 is all ones), row-major.  With syn_j = encode(data)_j ^
 * stored parity_j, data shard c explains a byte column iff syn_j == R[j][c] * syn_0 for every
 * j >= 1, and parity shard j iff syn_i == 0 for every i != j; the locate kernels' tables are
 * built from R. */
int rsmi_locate_matrix(const rsmi_ctx* ctx, uint8_t* out);

/* ------------------------------------------------------------------ locate pair: which two shards are wrong */

/* Locate stops at one culprit; with m >= 3 the code can name two.  Let n = k + m and H = [M | I_m],
 * M the m x k parity part of the encode matrix: column h_x of H is M[.][x] for a data shard x and
 * the unit vector of row j for parity shard k + j.  syn is Verify's syndrome vector per byte column
 * over bytes [0, S).
 *   Explaining pair.  A pair {x, y}, x < y, explains a stripe iff at every byte column syn lies in
 *   span{h_x, h_y}; equivalently, replacing rows x and y by their reconstruction from the other
 *   rows yields a clean stripe.  Padding never counts.
 *   Verdict.  Two int32 per block, out[2b] and out[2b+1]:
 *     (-1, -1)       the stripe is clean;
 *     (x, -1)        rsmi_locate names the single shard x (unchanged from rsmi_locate; no pair test
 *                    is run for such a block);
 *     (x, y), x < y  no single shard explains the stripe and exactly one pair does;
 *     (-2, -2)       every other case.
 *   For m >= 2 rsmi_locate's UNKNOWN means that no single shard explains the stripe, so every
 *   explaining pair found behind it is a genuine pair.
 * What the code's distance (m + 1) gives -- a property of the code, not of the implementation:
 *   m <= 2        no pair is ever named: every pair explains everything.  Such contexts get
 *                 rsmi_locate's verdicts widened to two words;
 *   m = 3         a pair is named when it happens to be the only one; that is not guaranteed;
 *   m >= 4        two damaged shards are always named;
 *   three or more damaged shards: the verdict is (-2, -2), or the damage imitates a pair, which
 *                 is then that block's unique explanation.
 * A named pair is repaired by rsmi_reconstruct_mixed_batch_* with the two shards absent and
 * required.  Layout, argument checks, their order and their statuses are those of rsmi_locate_*.
 * The calls are joined to ABI version 5 (additive); none of them takes or clears the per-thread
 * wait hook. */

/* Device-resident.  d_pair_out (device memory, 2 * nblocks verdict words) and, when d_bad_out is not
 * NULL, d_bad_out[b*m + j], exactly rsmi_verify_batch_dev's flags.  Nothing else is written.
 * Stream-ordered, no sync (scratch is kept per stream; growing it waits for that stream once). */
int rsmi_locate_pair_batch_dev(rsmi_ctx* ctx, const uint8_t* d_data, size_t data_shard_stride,
                               size_t data_block_stride, const uint8_t* d_parity, size_t parity_shard_stride,
                               size_t parity_block_stride, size_t S, size_t nblocks, int32_t* d_pair_out,
                               uint32_t* d_bad_out, void* stream);

/* Host memory, layout and the three paths of rsmi_verify_batch_host; pair_out[2b], pair_out[2b+1]
 * and (when not NULL) bad_out[b*m + j] in host memory. */
int rsmi_locate_pair_batch_host(rsmi_ctx* ctx, const uint8_t* data, size_t data_block_stride, const uint8_t* parity,
                                size_t parity_block_stride, size_t S, size_t nblocks, int32_t* pair_out,
                                uint32_t* bad_out);

/* One block of n*S contiguous bytes: pair_out[0], pair_out[1] receive its verdict. */
int rsmi_locate_pair(rsmi_ctx* ctx, const uint8_t* shards, size_t S, int pair_out[2]);

/* Host-only, works without a GPU: m - 2 linearly independent rows c_i (m bytes each, row-major in
 * out) with c_i . h_x = c_i . h_y = 0, so {x, y} explains a byte column iff every c_i . syn = 0.
 * The pair kernels' tables are built from these rows.  m <= 2: nothing is written, RSMI_OK.
 * x == y or an index outside [0, n): RSMI_ERR_INVALID_ARG. */
int rsmi_locate_pair_checks(const rsmi_ctx* ctx, int x, int y, uint8_t* out);

/* ------------------------------------------------------------------ heal: rewrite the shard that is wrong */

/* Locate names the shard that breaks a stripe; heal goes on, on the same stream and with no host
 * round trip in between, to rewrite it, so a scrub needs no sort of the blocks by culprit and no
 * reconstruct call per erasure pattern: every dirty block may have its own culprit.
 *   Outputs.  culprit_out[b] and the optional bad_out are exactly what rsmi_locate_* returns for
 *   the stripes as they were before the call.
 *   What is written.  In every block whose verdict is a shard x in [0, k+m), bytes [0, S) of row x
 *   are rewritten so that the stripe is clean: the new row is the reconstruction of row x from the
 *   other rows.  Blocks whose verdict is RSMI_LOCATE_CLEAN or RSMI_LOCATE_UNKNOWN are not written
 *   at all.  No row other than x is written, no byte at or past S of any row, no byte of a gap:
 *   the layout contract holds, padding may be read and is never written.  m = 1 never heals: a
 *   dirty stripe there is always UNKNOWN.
 *   What the code's distance (m + 1) gives -- a property of the code, not of the implementation:
 *   with at most m - 1 damaged shards in a block a named shard is the only damaged one, and the
 *   heal restores the original bytes.  With m or more damaged shards the damage can imitate a
 *   single other shard (see locate above); the heal then rewrites that shard: the stripe becomes
 *   a clean codeword, but not the original one.  Callers that cannot bound the damage keep the
 *   shard checksums as the second witness.
 *   Overlap.  The data and parity halves must not overlap each other.
 * Argument checks and statuses are those of rsmi_locate_*.  The calls are joined to ABI version 5
 * (additive); none of them takes or clears the per-thread wait hook. */

/* Device-resident: layout, argument checks and fast-path alignment as rsmi_locate_batch_dev.
 * Stream-ordered, no sync: d_culprit_out is written by the locate launches and read by the heal
 * launch behind them on the stream (scratch is kept per stream; growing it waits for that stream
 * once). */
int rsmi_heal_batch_dev(rsmi_ctx* ctx, uint8_t* d_data, size_t data_shard_stride, size_t data_block_stride,
                        uint8_t* d_parity, size_t parity_shard_stride, size_t parity_block_stride, size_t S,
                        size_t nblocks, int32_t* d_culprit_out, uint32_t* d_bad_out, void* stream);

/* Host memory, layout and the three paths of rsmi_verify_batch_host; culprit_out[b] and (when not
 * NULL) bad_out[b*m + j] in host memory.  Page-locked data and parity are healed where they lie,
 * by kernel stores over PCIe; from the staging of a small call and from the device rows of the
 * upload pipeline the rewritten rows are copied back to the caller's buffers, and nothing else. */
int rsmi_heal_batch_host(rsmi_ctx* ctx, uint8_t* data, size_t data_block_stride, uint8_t* parity,
                         size_t parity_block_stride, size_t S, size_t nblocks, int32_t* culprit_out,
                         uint32_t* bad_out);

/* One block of n*S contiguous bytes, healed in place: *culprit_out receives its verdict. */
int rsmi_heal(rsmi_ctx* ctx, uint8_t* shards, size_t S, int* culprit_out);

/* ------------------------------------------------------------------ heal pair: rewrite the two shards that are wrong */

/* Locate pair names the two shards that break a stripe; heal pair goes on, on the same stream and
 * with no host round trip in between, to rewrite them.  One call locates singles and pairs and
 * rewrites every named shard; every dirty block may have its own pair.  Blocks that come back
 * (-2, -2) are untouched and go to the caller's slow path.
 *   Outputs.  pair_out and the optional bad_out are exactly what rsmi_locate_pair_* returns for the
 *   stripes as they were before the call.
 *   What is written.  Verdict (x, -1): bytes [0, S) of row x are rewritten exactly as rsmi_heal
 *   rewrites them.  Verdict (x, y): bytes [0, S) of rows x and y are rewritten to their
 *   reconstruction from the other n - 2 rows, so the stripe is clean.  Blocks with (-1, -1) or
 *   (-2, -2) are not written at all.  No other row is written, no byte at or past S of any row, no
 *   byte of a gap: the layout contract holds, padding may be read and is never written.
 *   What the code's distance (m + 1) gives -- a property of the code, not of the implementation:
 *     m <= 2   the call is rsmi_heal with its verdicts widened to two words;
 *     m = 3    a pair is healed when it is the block's only explanation; that is not guaranteed;
 *     m >= 4   two damaged shards get their original bytes back;
 *   with three or more damaged shards the damage can imitate a pair; the heal then makes a clean
 *   codeword that is not the original.  Callers that cannot bound the damage keep the shard
 *   checksums as the second witness.
 *   Overlap.  The data and parity halves must not overlap each other.
 * Layout, argument checks, their order and their statuses are those of rsmi_locate_pair_*; the
 * shards are writable, as in rsmi_heal_*.  The calls are joined to ABI version 5 (additive); none
 * of them takes or clears the per-thread wait hook. */

/* Device-resident.  Stream-ordered, no sync: d_pair_out is written by the locate pair launches and
 * read by the heal launch behind them on the stream (scratch is kept per stream; growing it waits
 * for that stream once). */
int rsmi_heal_pair_batch_dev(rsmi_ctx* ctx, uint8_t* d_data, size_t data_shard_stride, size_t data_block_stride,
                             uint8_t* d_parity, size_t parity_shard_stride, size_t parity_block_stride, size_t S,
                             size_t nblocks, int32_t* d_pair_out, uint32_t* d_bad_out, void* stream);

/* Host memory, layout and the three paths of rsmi_verify_batch_host; pair_out[2b], pair_out[2b+1]
 * and (when not NULL) bad_out[b*m + j] in host memory.  Page-locked data and parity are healed
 * where they lie; from the staging of a small call and from the device rows of the upload pipeline
 * the one or two rewritten rows of a block are copied back to the caller's buffers, and nothing
 * else. */
int rsmi_heal_pair_batch_host(rsmi_ctx* ctx, uint8_t* data, size_t data_block_stride, uint8_t* parity,
                              size_t parity_block_stride, size_t S, size_t nblocks, int32_t* pair_out,
                              uint32_t* bad_out);

/* One block of n*S contiguous bytes, healed in place: pair_out[0], pair_out[1] receive its verdict. */
int rsmi_heal_pair(rsmi_ctx* ctx, uint8_t* shards, size_t S, int pair_out[2]);

/* Host-only, works without a GPU: the 2 x m matrix D (row-major in out) with D h_x = (1, 0)^T and
 * D h_y = (0, 1)^T for the columns of H = [M | I_m].  With syn Verify's syndrome vector, D syn is
 * (row x's error, row y's error) at every byte column that {x, y} explains.  D is the form the
 * kernels use, with at most two non-zero columns l0, l1:
 *   {k+i, k+j}   the unit rows i, j;
 *   {c, k+j}     l = 0 (1 when j = 0): e_c = syn_l / M[l][c], e_{k+j} = syn_j ^ M[j][c] e_c;
 *   {c, d}       the inverse of the 2 x 2 minor of rows 0, 1 (non-singular for every pair: M is MDS).
 * D [h_x h_y] = I_2 is what makes the kernels' update idempotent per byte.  On layouts whose rows
 * are not 16-byte aligned a row's last 16-byte window overlaps the one before it, and the two may
 * be healed by different waves: a wave that sees row x healed already and row y not forms
 * syn = h_y e_y and gets the deltas (0, e_y).  That holds because each byte's deltas come from the
 * same loads as its syndromes: no byte is loaded twice.
 * x == y, an index outside [0, n) or m < 2: RSMI_ERR_INVALID_ARG. */
int rsmi_heal_pair_matrix(const rsmi_ctx* ctx, int x, int y, uint8_t* out);

/* Erasure.EncodeData for one block (same output as rsmi_encode_block, plus R(shard) in
 * raw_out[0..k+m) when raw_out is not NULL), coalesced with concurrent callers on the same
 * context: DagNode.Put runs once per block from many goroutines (node.go:358-408), and
 * group commit turns those calls into GPU batches.  A caller whose block is still queued and
 * that finds one of the context's "coalesce_lanes" lanes free (default 2) executes every block
 * queued so far (waiting up to option "coalesce_us" for more, default 0; at most
 * "coalesce_max" blocks, default 256) and wakes the others; blocks arriving while every lane
 * codes a batch form the next one.  Lane i > 0 codes on a child context of its own (streams and
 * scratch), so one batch is launched while the one before it runs.  A batch whose blocks lie in
 * page-locked memory (rsmi_host_alloc) is coded in place, up to 64 blocks per launch.  A lone
 * caller never waits on anyone.  block may be
 * shards_out itself: the caller has already copied the block to the start of shards_out
 * (Split's copy, done on the caller's own thread), and the engine zero-pads and encodes it in
 * place; any other overlap of block and shards_out is not allowed. */
int rsmi_encode_block_coalesced(rsmi_ctx* ctx, const uint8_t* block, size_t B, uint8_t* shards_out,
                                uint32_t* raw_out);

/* rsmi_encode_block_coalesced with the mutcask CRC-32 as well: raw32_out[0..k+m) = R32(shard)
 * when not NULL (see "mutcask CRC-32" below); raw16_out as raw_out above. */
int rsmi_encode_block_coalesced_crcs(rsmi_ctx* ctx, const uint8_t* block, size_t B, uint8_t* shards_out,
                                     uint32_t* raw16_out, uint32_t* raw32_out);

/* rsmi_reconstruct (same arguments, results and errors), coalesced the same way.  When a
 * datanode is down every concurrent DagNode.Get misses the same shard (node.go:277-282), so
 * concurrent degraded reads share one erasure pattern and batch into one launch; requests
 * with different shard sizes or patterns run as separate groups of the same batch. */
int rsmi_reconstruct_coalesced(rsmi_ctx* ctx, uint8_t* shards, size_t S, const uint8_t* present, int data_only);

/* Counters: "coalesced_calls", "coalesced_batches" (both coalesced entry points); diagnostic:
 * "coalesced_wakes", the wake-ups of callers that slept, and "coalesced_wake_ns", the summed time
 * from each wake-up call to the caller running again.  "launch_units_max": the value of that
 * option in force.  "split_launches": the kernel launches issued so far by the loops that cut a
 * batch at "launch_units_max" (encode and reconstruct, the fused encode + CRC-16, the stripe
 * checks' tile launches, scrub's unit launches, the mixed reconstruct's class launches), by this
 * context and its coalescing lanes; a call that ran in one piece adds one per kernel, a call that
 * was cut adds one per piece.  -1 for an unknown key. */
long rsmi_get_stat(const rsmi_ctx* ctx, const char* key);

/* A host task for the calling thread to run while its next codec call's device work is in
 * flight.  DagNode.Put (node.go:376-399) encodes and then writes every shard; the data shards
 * that hold only block bytes are final once Split, so the host mirror writes them to their
 * datanodes while the GPU encodes the parity, on the calling thread, without a hand-off.  The
 * hook is per thread and one-shot: the next rsmi_encode_block_coalesced(_crcs),
 * rsmi_reconstruct_coalesced, or one-block host call of rsmi_encode_batch_host(_crcs),
 * rsmi_reconstruct_batch_host or rsmi_reconstruct_rows_batch_host(_crcs) that runs as one
 * in-place kernel (page-locked rows, or a small call) on this thread
 * takes it and runs fn(arg) once on this thread -- after its device work is launched and before
 * it waits for it, or, when the call has no work of its own in flight at that point (a caller whose
 * block another thread's batch codes), before it blocks.  A call may hold the context's lock while
 * fn runs, so fn must make no codec call (host-only helpers such as the CRC folds are fine) and
 * must not throw.  Other entry points, calls that take the copy-engine pipeline and calls that
 * fail before launching leave the hook pending.  fn == NULL clears it.  A lone DagNode.Get uses it
 * too: it copies the block's present data rows while the GPU rebuilds the missing ones. */
void rsmi_set_wait_hook(void (*fn)(void*), void* arg);

/* Run the calling thread's hook if it is still pending (no call took it) and clear it: 1 if it
 * ran, 0 if there was none.  Setting a hook, making the call and then calling this runs the
 * task exactly once whatever path the call took. */
int rsmi_run_wait_hook(void);

/* ------------------------------------------------------------------ datanode CRC-16 */

/* The datanode stores every shard as |crc (4 LE)|meta size|data size|meta|data| with
 * crc = howeyc/crc16 Checksum(entry[4:], IBMTable) (dag/node/datanode/server.go:58-75),
 * and re-checks it on Get / GetMeta (server.go:93-97, :115-119).  These entry points move
 * the byte-serial CRC over the shard bytes onto the GPU; the host
 * only folds in the 12-byte header.  "Raw" CRC R(D) = the CRC-16 register after D from a
 * zero register, no complement (reflected polynomial 0xA001), held in a uint32. */

/* howeyc Checksum(p, IBMTable) on the host (carry-less-multiply folding from 256 bytes where the
 * CPU has VPCLMULQDQ, ~30 GiB/s per core; slice-by-8 otherwise).  Replaces the datanode's
 * crc16.Checksum(entry[4:], IBMTable) (dag/node/datanode/server.go:70, :93-97). */
uint16_t rsmi_crc16_ibm(const uint8_t* p, size_t n);

/* Checksum(head || D) from R(D) and |D|: with head = |meta size (4 LE)|data size (4 LE)|meta|
 * this is the entry checksum server.go:70 computes for a shard D.  head may be empty. */
uint16_t rsmi_crc16_entry(const uint8_t* head, size_t head_len, uint32_t raw, size_t data_len);

/* R(row) for nrows rows of S bytes per block on the device: row r of block b at
 * d_rows + b*block_stride + r*shard_stride; d_raw_out[b*out_block_stride + r] is zeroed and
 * then receives R(row).  Any alignment (16-byte aligned rows take the fast path).
 * Stream-ordered. */
int rsmi_crc16_rows_dev(rsmi_ctx* ctx, const uint8_t* d_rows, size_t shard_stride, size_t block_stride, int nrows,
                        size_t S, size_t nblocks, uint32_t* d_raw_out, size_t out_block_stride, void* stream);

/* rsmi_encode_batch_host plus R(shard) of every shard it touched, computed on the GPU from
 * the rows already resident there: raw_out[b*(k+m) + r] for data rows r < k and parity rows
 * k <= r < k+m.  DagNode.Put / PutMany hand these to the datanodes, which then store the
 * entry without a host CRC pass. */
int rsmi_encode_batch_host_crc(rsmi_ctx* ctx, const uint8_t* data, size_t data_block_stride, uint8_t* parity,
                               size_t parity_block_stride, size_t S, size_t nblocks, uint32_t* raw_out);

/* rsmi_encode_batch_dev with the CRC fused into the encode pass: every row the kernel reads
 * or writes is folded into per-chunk CRC-16 values on the way, and a combine pass writes
 * d_raw_out[b*(k+m) + r] = R(shard r of block b) (device memory).  The SURVEY.md 8(f) rank 2
 * form: no second pass over the shard bytes.  Stream-ordered. */
int rsmi_encode_batch_dev_crc(rsmi_ctx* ctx, const uint8_t* d_data, size_t data_shard_stride,
                              size_t data_block_stride, uint8_t* d_parity, size_t parity_shard_stride,
                              size_t parity_block_stride, size_t S, size_t nblocks, uint32_t* d_raw_out,
                              void* stream);

/* rsmi_encode_block plus raw_out[r] = R(shard r), r < k+m. */
int rsmi_encode_block_crc(rsmi_ctx* ctx, const uint8_t* block, size_t B, uint8_t* shards_out, uint32_t* raw_out);

/* R(row) (raw16_out) and/or R32(row) (raw32_out, mutcask CRC-32) of nrows host rows of S bytes,
 * row r at rows + r*row_stride; page-locked rows (rsmi_host_alloc) are read in place over
 * PCIe.  The Dag Node's GPU-verified reads check fetched shards against the checksums the
 * datanodes stored (server.go:93-97 moved to the reader); either output may be NULL. */
int rsmi_crc_rows_host(rsmi_ctx* ctx, const uint8_t* rows, size_t row_stride, size_t nrows, size_t S,
                       uint32_t* raw16_out, uint32_t* raw32_out);

/* ------------------------------------------------------------------ mutcask CRC-32 */

/* The mutcask KV engine under a datanode (kv/mutcask/cask.go:73-97, selected by
 * server.go:207) stores every value as |crc32 (4 LE)|value| with crc32 = Go
 * crc32.ChecksumIEEE(value) (the zlib CRC-32), and re-checks it on every read (cask.go:250).
 * The value is the datanode's whole entry, so the shard bytes get a second byte-serial pass
 * on every Put and Get.  "Raw" R32(D) = the CRC-32 register after D from a zero register,
 * no complement (reflected polynomial 0xEDB88320). */

/* crc32.ChecksumIEEE(p) on the host (the same folding).  Replaces the mutcask engine's
 * crc32.ChecksumIEEE (kv/mutcask/cask.go:73-79, :250). */
uint32_t rsmi_crc32_ieee(const uint8_t* p, size_t n);

/* ChecksumIEEE(head || D) from R32(D) and |D|: with head = the datanode entry's first 12 + meta
 * bytes (|crc16 (4 LE)|meta size|data size|meta|) this is the mutcask value checksum of a
 * shard D's entry.  head may be empty.  Any data_len is accepted (the shift by |D| counts
 * modulo 2^32 - 1, the order of the zero-byte step); only the device passes limit a row, to
 * below 4 GiB. */
uint32_t rsmi_crc32_entry(const uint8_t* head, size_t head_len, uint32_t raw, size_t data_len);

/* R32(row) for nrows rows of S bytes per block on the device, laid out as in
 * rsmi_crc16_rows_dev (d_raw_out[b*out_block_stride + r], zeroed first).  Stream-ordered. */
int rsmi_crc32_rows_dev(rsmi_ctx* ctx, const uint8_t* d_rows, size_t shard_stride, size_t block_stride, int nrows,
                        size_t S, size_t nblocks, uint32_t* d_raw_out, size_t out_block_stride, void* stream);

/* rsmi_encode_batch_host with either or both raw checksums of every shard it touched:
 * raw16_out[b*(k+m) + r] = R(shard) (CRC-16, as rsmi_encode_batch_host_crc) and
 * raw32_out[b*(k+m) + r] = R32(shard) (CRC-32), each optional (NULL).  The CRC-32 pass reads
 * the rows where the encode left them (device staging, or page-locked host memory on the
 * zero-copy path).  DagNode.PutMany hands both to mutcask-backed datanodes. */
int rsmi_encode_batch_host_crcs(rsmi_ctx* ctx, const uint8_t* data, size_t data_block_stride, uint8_t* parity,
                                size_t parity_block_stride, size_t S, size_t nblocks, uint32_t* raw16_out,
                                uint32_t* raw32_out);

/* rsmi_reconstruct_batch_host (same arguments, results and errors) that also returns R(row), the
 * datanode CRC-16 of the entry's shard bytes, of the k survivor rows it read: raw16_in[b*k + c] =
 * R(shard used[c]), used = the first k present shards (rsmi_decode_matrix's used_rows).  A
 * reader that fetched shards unchecked (the datanodes' stored checksums, server.go:93-97) checks
 * them for free on a degraded read: with page-locked shards one kernel reads each survivor once
 * for both; otherwise a CRC pass over the survivors follows the rebuild. */
int rsmi_reconstruct_batch_host_verify(rsmi_ctx* ctx, uint8_t* shards, size_t block_stride, size_t S, size_t nblocks,
                                       const uint8_t* present, int data_only, uint32_t* raw16_in);

/* rsmi_reconstruct_rows_batch_host plus the raw checksums of every row it rebuilt, from the
 * GPU where the rows land: raw16_out / raw32_out[b*(k+m) + r] = R(row) / R32(row) for rows r
 * that are required and missing, 0 for the others; either may be NULL.  RepairDataNode's
 * Puts of the rebuilt rows (data_recovery.go:102-106) then carry sender checksums like
 * DagNode.Put's. */
int rsmi_reconstruct_rows_batch_host_crcs(rsmi_ctx* ctx, uint8_t* shards, size_t block_stride, size_t S,
                                          size_t nblocks, const uint8_t* present, const uint8_t* required,
                                          uint32_t* raw16_out, uint32_t* raw32_out);

/* ------------------------------------------------------------------ checksums of named rows */

/* The calls that rewrite rows on the device (rsmi_heal_batch_dev, rsmi_heal_pair_batch_dev, the
 * mixed reconstruct) write a different set of rows in every block.  The checksums of exactly those
 * rows are the second witness of a heal (R(healed row) against the stored entry checksum shows a
 * clean codeword that is not the original) and the sender checksums of a repaired shard's Put.
 *
 * R(row) and/or R32(row) of the rows a device array names, per block.  Layout and fast-path
 * alignment as rsmi_verify_batch_dev (two halves: row r < k in the data half, row k + j in the
 * parity half).  d_rows: DEVICE memory, nblocks * slots int32, read on the stream, so an array
 * written by an earlier launch on that stream (rsmi_heal_batch_dev's d_culprit_out with slots 1,
 * rsmi_heal_pair_batch_dev's d_pair_out with slots 2) is consumed with no host round trip.  An
 * entry in [0, k+m) names that row of its block; every other value (RSMI_LOCATE_CLEAN,
 * RSMI_LOCATE_UNKNOWN, anything out of range) names nothing, and no address is formed from it.
 * d_raw16_out / d_raw32_out[b*slots + s] (device memory, either may be NULL, not both; zeroed on
 * the stream first) = R / R32 over bytes [0, S) of the row entry (b, s) names, 0 where it names
 * nothing; rsmi_crc16_entry / rsmi_crc32_entry finish them on the host.  Nothing else is written;
 * only named rows are read (padding of a named row may be read, as everywhere).  The same row may
 * be named twice.  Stream-ordered, no sync; the wait hook is neither taken nor cleared.
 * Arguments: rsmi_verify_batch_dev's checks first, in its order and with its statuses; then
 * d_rows == NULL, slots outside [1, k+m] or both outputs NULL -> RSMI_ERR_INVALID_ARG; a row of
 * 4 GiB or more with d_raw32_out set -> RSMI_ERR_INVALID_ARG (as rsmi_crc32_rows_dev); nblocks == 0
 * -> RSMI_OK; all before any device access. */
int rsmi_crc_named_rows_dev(rsmi_ctx* ctx, const uint8_t* d_data, size_t data_shard_stride, size_t data_block_stride,
                            const uint8_t* d_parity, size_t parity_shard_stride, size_t parity_block_stride, size_t S,
                            size_t nblocks, const int32_t* d_rows, int slots, uint32_t* d_raw16_out,
                            uint32_t* d_raw32_out, void* stream);

/* ------------------------------------------------------------------ device groups (several GPUs, one process) */

/* The Dag Pool runs every DagNode of a cluster in one process (dag/pool/poolservice/cluster.go:
 * 28-41).  A device group is one context per entry of devices[] (an entry may repeat: two
 * contexts on one GPU overlap their copies and kernels).  Its batch calls split the blocks
 * into contiguous ranges, one per member, sizes differing by at most one block (rsmi_partition),
 * and run every range on its member's context from its own host thread -- no data crosses
 * devices, no collective runs -- then return the first failing member's status in member
 * order.  Same arguments, layouts, results and errors as the single-context calls (nblocks == 0
 * validates the arguments on member 0 and returns).  Each member's thread is persistent and
 * bound to its GPU's NUMA node (CPUs and preferred memory), so the page-locked staging its
 * context allocates sits on that socket; one batch call runs at a time per group. */
typedef struct rsmi_group rsmi_group;
int rsmi_group_open(int k, int m, const int* devices, int ndev, rsmi_group** out);
void rsmi_group_close(rsmi_group* group);
int rsmi_group_size(const rsmi_group* group);
/* Member i's context (owned by the group), for the single-context calls; NULL if out of range. */
rsmi_ctx* rsmi_group_context(rsmi_group* group, int i);
/* The range of blocks member i of parts codes: contiguous, sizes differ by at most one. */
int rsmi_partition(size_t nblocks, int parts, int i, size_t* start, size_t* count);
/* keyHashSlot (dag/pool/poolservice/hash_slot.go:20-22): howeyc crc16 IBM of the key & 0x3FFF. */
int rsmi_key_slot(const uint8_t* key, size_t len);
/* The member that owns a key: contiguous slot ranges of 16384 / size slots per member, as
 * DagNodes own SlotPairs -- a stable key -> GPU map for per-block callers. */
int rsmi_group_member_of_key(const rsmi_group* group, const uint8_t* key, size_t len);
/* Member i's NUMA node (rsmi_device_numa_node of its device), -1 if unknown. */
int rsmi_group_member_numa_node(const rsmi_group* group, int i);
/* Page-locked (portable, mapped) host memory for nblocks blocks of block_bytes whose member
 * ranges (rsmi_partition over the group's size) sit on the members' NUMA nodes, so on the
 * zero-copy path each member's DMA reads and writes only its own socket's memory.  Zeroed.
 * Freed by rsmi_group_host_free or rsmi_group_close.  NULL on failure. */
void* rsmi_group_host_alloc(rsmi_group* group, size_t block_bytes, size_t nblocks);
void rsmi_group_host_free(rsmi_group* group, void* p);
/* The host NUMA node closest to a device: hipDeviceAttributeHostNumaId, else sysfs
 * bus/pci/devices/<pci bus id>/numa_node; -1 when unknown. */
int rsmi_device_numa_node(int device);
/* Host-only helpers behind it, with the sysfs root injectable ("/sys" in production): the
 * numa_node of a PCI bus id ("0000:75:00.0", any case; -1 if absent), and a node's CPU list
 * (devices/system/node/node<N>/cpulist: returns the number of CPUs, writes at most max_cpus;
 * -1 if absent or malformed). */
int rsmi_sysfs_numa_node(const char* sysfs_root, const char* pci_bus_id);
int rsmi_sysfs_node_cpus(const char* sysfs_root, int node, int* cpus, int max_cpus);
/* Bind the calling thread to a NUMA node: the node's CPUs the process may use, and a
 * preferred-node memory policy (allocations fall back to other nodes, never fail). */
int rsmi_bind_thread_to_numa_node(int node);
int rsmi_group_encode_batch_host(rsmi_group* group, const uint8_t* data, size_t data_block_stride, uint8_t* parity,
                               size_t parity_block_stride, size_t S, size_t nblocks);
int rsmi_group_encode_batch_host_crcs(rsmi_group* group, const uint8_t* data, size_t data_block_stride, uint8_t* parity,
                                    size_t parity_block_stride, size_t S, size_t nblocks, uint32_t* raw16_out,
                                    uint32_t* raw32_out);
int rsmi_group_reconstruct_batch_host(rsmi_group* group, uint8_t* shards, size_t block_stride, size_t S, size_t nblocks,
                                    const uint8_t* present, int data_only);
int rsmi_group_reconstruct_rows_batch_host(rsmi_group* group, uint8_t* shards, size_t block_stride, size_t S,
                                         size_t nblocks, const uint8_t* present, const uint8_t* required);

/* ------------------------------------------------------------------ tuning / introspection */

/* Options: "waves_per_cu" (grid cap; 0 = the default geometry: one tile per wave for the
 * coding kernels, 48/96 waves per CU for the CRC rows passes), "launch_units_max" (the most tiles
 * -- 1 KiB of every row of a block -- or, for the fused encode + CRC-16 and scrub, units of 4 tiles
 * that one kernel launch takes; a longer batch runs as several launches of whole blocks, a block
 * never being cut; 1 to 2^24 - 1, which is the default and keeps every launch below 2^32 threads;
 * 0 = the default; a table launch of a coalesced group that would pass it runs per block),
 * "zero_copy" (1 = default: host
 * batch calls whose buffers are page-locked (rsmi_host_alloc) run as one kernel that reads and
 * writes them in place over PCIe, at any size; 2 = the same, also reading inputs in place on
 * the pipeline path; 0 = always the copy-engine pipeline), "small_call_bytes" (host calls moving
 * at most this many shard bytes, default 2 MiB, run as one such kernel -- pageable buffers are
 * staged through a page-locked one by CPU copies; 0 = never), "coalesce_us" / "coalesce_max"
 * (rsmi_encode_block_coalesced), "crc16_fold" (the CRC-16 rows pass on 16-byte-aligned rows:
 * 1 = default, the fold on the matrix cores (fp4 MFMA); 0 = the nibble-table fold; both
 * bit-exact), "crc16_fused_fold" (the encode with the CRC-16 fused in, on
 * 16-byte-aligned layouts: 1 = default, rs_fused_mfma_kernel folds on the matrix cores; 0 = the
 * nibble-table variants), "crc32_fold" (the mutcask CRC-32 rows pass: 1 = the fold on the
 * matrix cores, 0 = the nibble-table fold; both bit-exact), "inject_host_fault" (test hook: the
 * next N coalesced batches, or direct rsmi_encode_batch_host* calls, throw std::bad_alloc, so their
 * requests return RSMI_ERR_HOST; default 0), "inject_lane_fault" (test hook: the next N coalescing lane contexts
 * fail to open, as a device error would; default 0), "coalesce_lanes" (coalesced batches coded at
 * once, 1-16, default 2; every option but the test hooks also applies to the lanes' child
 * contexts), "coalesce_carry"
 * (batches a lane's executor goes on to when they are queued by the time its own completes,
 * before it hands the lane to a waiting caller, 0-16, default 1), "coalesce_pipeline" (1 =
 * default: a coalesced batch coded by the table kernels is left in flight behind an event while
 * the lane's next queued batch is launched behind it, and its callers return when the event
 * completes; 0 = every batch synchronises before the next is launched), "coalesce_flag" (1 =
 * default: a coalesced group coded by one table launch of the encode + CRC-16, and a one-block
 * in-place host call (encode + CRC-16, reconstruct, verified reconstruct), signal their end through
 * a page-locked flag the launch's last workgroup releases, which the caller polls instead of
 * synchronising -- blocking in the synchronisation after 200 us; 0 = event / stream
 * synchronisation).  Kernel variants measured slower than the defaults are not
 * built into the library.  Returns RSMI_ERR_INVALID_ARG for unknown keys or
 * values. */
int rsmi_set_option(rsmi_ctx* ctx, const char* key, long value);
/* Name of the kernel the last device launch on this context used ("" if none); a copy owned by
 * the calling thread, valid until its next rsmi_last_kernel call. */
const char* rsmi_last_kernel(const rsmi_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* RSMI_H */
