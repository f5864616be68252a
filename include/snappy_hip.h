/*
 * snappy_hip.h -- C ABI of libsnappy_hip.so, the MI355X (gfx950) drop-in for the
 * UPMEM-DPU offload path of UBC-ECE-Sasha/PIM-compression's `dpu_snappy`.
 *
 * Two layers are exported:
 *
 *  1. The drop-in pair, with the exact shape of the reference's L2 entry points
 *       snappy_compress_dpu    (reference snappy/snappy_compress.h:37,  snappy_compress.c:487)
 *       snappy_decompress_dpu  (reference snappy/snappy_decompress.h:34, snappy_decompress.c:292)
 *     They take the reference's own `struct host_buffer_context` /
 *     `struct program_runtime` (reference snappy/dpu_snappy.h:37-55) and return its
 *     `snappy_status` (dpu_snappy.h:21-25).  `main` in dpu_snappy.c:169-172 / :189-192
 *     calls them where it called the *_dpu functions.
 *
 *  2. A resident API over device pointers (what the drop-in pair is built from, and what
 *     bench.py / the tests drive): per-block compress into worst-case slots, scan+compact
 *     into the framed stream, size-chain indexing, per-block decompress.  It replaces the
 *     dpu_alloc / dpu_push_xfer / dpu_launch plumbing (snappy_compress.c:535-618,
 *     snappy_decompress.c:351-439) with hipMalloc / hipMemcpy / kernel launches.
 *
 * Plain C: pointers and sizes only.  No CPU fallback exists behind any entry point: if no
 * HIP device / code object is usable they fail with SNAPPY_HIP_ERR_* (resident API) or
 * SNAPPY_INVALID_INPUT (drop-in pair, as the reference maps a failed dpu_launch,
 * snappy_compress.c:618-623) and say why on stderr / via snappy_hip_last_error().
 */
#ifndef SNAPPY_HIP_H_
#define SNAPPY_HIP_H_

#include <stdint.h>
#include <stddef.h>

/* The library is built with -fvisibility=hidden: the functions declared in this header are its whole dynamic symbol table. */
#if defined(__GNUC__)
#define SNAPPY_HIP_API __attribute__((visibility("default")))
#else
#define SNAPPY_HIP_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- types shared with the reference (layout-identical; skipped when the
 *      reference's own dpu_snappy.h was included first) ------------------- */
#ifndef _DPU_SNAPPY_H_
typedef enum {
	SNAPPY_OK = 0,
	SNAPPY_INVALID_INPUT,
	SNAPPY_BUFFER_TOO_SMALL
} snappy_status;                        /* dpu_snappy.h:21-25 */

typedef struct host_buffer_context {
	const char *file_name;
	uint8_t *buffer;
	uint8_t *curr;
	unsigned long length;
	unsigned long max;
} host_buffer_context;                  /* dpu_snappy.h:37-44 */

struct program_runtime {
	double pre;
	double d_alloc;
	double load;
	double copy_in;
	double run;
	double copy_out;
	double d_free;
};                                      /* dpu_snappy.h:47-55 */
#endif

/* ---- 1. drop-in pair ----------------------------------------------------- */

/*
 * Replaces snappy_compress_dpu (snappy_compress.c:487-714).
 * Entry: input->buffer/curr at file start, input->length = n.  output->buffer may be NULL
 * or any malloc'd block; it is realloc'd to the needed size (the reference's
 * 32+n+n/6, snappy_compress.c:446-447, is too small for tiny block sizes).  If the caller
 * sets output->max to a finite capacity (anything but ULONG_MAX, the reference's default,
 * dpu_snappy.c:112), output->buffer is used as is -- e.g. a page-locked buffer -- and
 * SNAPPY_BUFFER_TOO_SMALL is returned if the stream does not fit.
 * Exit: framed stream in output->buffer[0..output->length); caller writes the file.
 * Fills every field of *runtime (pre is accumulated with +=, as snappy_compress.c:528).
 * Uses SNAPPY_HIP_NUM_GPUS devices (env, default: all visible), contiguous block ranges
 * per device (snappy_compress.c:494-520), host-side concat of per-device outputs.
 */
SNAPPY_HIP_API snappy_status snappy_compress_gpu(struct host_buffer_context *input, struct host_buffer_context *output,
                                  uint32_t block_size, struct program_runtime *runtime);

/*
 * Replaces snappy_decompress_dpu (snappy_decompress.c:292-493).
 * Entry (as left by setup_decompression, snappy_decompress.c:187-215): input->curr just
 * past the first varint; output->buffer malloc'd, output->length = uncompressed length.
 * Reads the block-size varint itself (snappy_decompress.c:300), walks the u32 size chain on
 * the host (:317-340), decodes block i into output->buffer + i*block_size (:330).
 * Stricter than the host decoder: a block that overruns its compressed size, its output
 * window, or references bytes before its own start yields SNAPPY_INVALID_INPUT.
 */
SNAPPY_HIP_API snappy_status snappy_decompress_gpu(struct host_buffer_context *input, struct host_buffer_context *output,
                                    struct program_runtime *runtime);

/* ---- 2. resident API ----------------------------------------------------- */

#define SNAPPY_HIP_OK            0
#define SNAPPY_HIP_ERR_NO_DEVICE 1   /* no usable HIP device / runtime */
#define SNAPPY_HIP_ERR_ARG       2   /* bad argument (alignment, sizes, null) */
#define SNAPPY_HIP_ERR_RUNTIME   3   /* a HIP call failed; see snappy_hip_last_error() */

/* per-block status written by the decompress kernel */
#define SNAPPY_HIP_BLOCK_OK        0u
#define SNAPPY_HIP_BLOCK_INVALID   1u

#define SNAPPY_HIP_MIN_BLOCK_SIZE  1u
#define SNAPPY_HIP_MAX_BLOCK_SIZE  65535u   /* u16 hash table entries, snappy_compress.c:347 */

/* Description of one framed stream for snappy_hip_index_streams. */
typedef struct snappy_hip_stream_desc {
	const uint8_t *stream;      /* device: start of the framed stream (its header)      */
	uint64_t stream_len;        /* bytes                                                  */
	uint64_t *block_offsets;    /* device out: offset of each block's u32 size prefix    */
	uint32_t *result;           /* device out: [0]=status (SNAPPY_HIP_BLOCK_*), [1]=blocks walked */
	uint32_t total_len;         /* uncompressed length from the header                    */
	uint32_t block_size;        /* from the header                                        */
	uint32_t header_len;        /* bytes of the two varints                               */
	uint32_t num_blocks;        /* ceil(total_len / block_size)                           */
} snappy_hip_stream_desc;

/* Page-locked host memory for callers that want PCIe-rate copies through the drop-in pair (the CLI reads its
 * input file straight into such a buffer).  NULL on failure. */
SNAPPY_HIP_API void *snappy_hip_host_alloc(size_t bytes);
SNAPPY_HIP_API void snappy_hip_host_free(void *p);

SNAPPY_HIP_API int snappy_hip_device_count(void);
SNAPPY_HIP_API int snappy_hip_set_device(int device);
SNAPPY_HIP_API const char *snappy_hip_last_error(void);
/* name of the code-object architecture this library was built for ("gfx950") */
SNAPPY_HIP_API const char *snappy_hip_arch(void);

/* Bytes reserved per block in the slot buffer: 16-byte multiple >= 4 + 32 + bs + bs/6
 * (u32 prefix + snappy_max_compressed_length, snappy_compress.c:55-60). */
SNAPPY_HIP_API uint32_t snappy_hip_slot_stride(uint32_t block_size);
SNAPPY_HIP_API uint64_t snappy_hip_num_blocks(uint64_t input_len, uint32_t block_size);
/* Upper bound of the framed stream for input_len bytes (header + all slots' payload). */
SNAPPY_HIP_API uint64_t snappy_hip_stream_bound(uint64_t input_len, uint32_t block_size);
/* Writes varint(total_len) varint(block_size) (snappy_compress.c:461-465) to a HOST buffer
 * of >= 10 bytes; returns header length. */
SNAPPY_HIP_API uint32_t snappy_hip_write_header(uint8_t *dst, uint32_t total_len, uint32_t block_size);
/* Parses the two header varints from a HOST buffer (snappy_decompress.c:193-198, :220-225);
 * returns header length, 0 if malformed. */
SNAPPY_HIP_API uint32_t snappy_hip_parse_header(const uint8_t *src, uint64_t avail, uint32_t *total_len, uint32_t *block_size);

/*
 * K1: compress every block of d_in independently (semantics of compress_block,
 * snappy_compress.c:284-413).  Block b's u32 size prefix + elements go to
 * d_slots + b*slot_stride; d_block_bytes[b] = 4 + compressed size.
 * d_in must be 16-byte aligned.  `stream` is a hipStream_t (NULL = default stream).
 *
 * d_scratch: 256-byte aligned device workspace of snappy_hip_compress_scratch_bytes() bytes (one 64 KiB
 * hash table per wavefront slot of the CURRENT device + a work counter: 512 MiB on a whole MI355X, 64 MiB on a
 * 32-CU partition -- the size is taken from hipGetDeviceProperties, so ask with the device selected that will
 * run the launch; contents need not be initialised, the buffer must not be shared by launches that run
 * concurrently).  If NULL or too small the LDS-table kernel is used instead (lower occupancy, same bytes).
 * After EVERY launch that was given a scratch, the u32 at byte 16 of the scratch holds the number of blocks that
 * were compressed by LDS-table wavefronts (statistics only): all of them when a small input went to the
 * LDS-table kernel alone, none with SNAPPY_HIP_LDS_WAVES=0.
 */
SNAPPY_HIP_API uint64_t snappy_hip_compress_scratch_bytes(void);
/* Wavefronts per CU whose hash table lives in LDS in a default K1 launch at this block size (the table is sized by the
 * block size, so small blocks get more of them: reference dpu_compress.c:16, :472-476 sizes its table to the tasklet's
 * memory the same way).  For the block-size sweep's occupancy column. */
SNAPPY_HIP_API uint32_t snappy_hip_k1_lds_waves_per_cu(uint32_t block_size);
SNAPPY_HIP_API int snappy_hip_compress_blocks(const uint8_t *d_in, uint64_t input_len, uint32_t block_size,
                               uint8_t *d_slots, uint32_t slot_stride, uint32_t *d_block_bytes,
                               void *d_scratch, uint64_t scratch_bytes, void *stream);

/*
 * K1 over a batch of containers in ONE launch: the same per-block semantics as snappy_hip_compress_blocks for every
 * item (its own input, slot array and size array; all with the same block_size and slot_stride), the persistent
 * wavefronts drawing blocks of all containers from one counter, so the batch has one tail instead of one per container.
 * This is the device-side form of the reference compressing many independent files, one `dpu_snappy -c` run each
 * (snappy/dpu_snappy.c:160-172); items is a HOST array, empty containers are skipped, lists longer than 8 non-empty
 * containers are issued as several launches on `stream`.
 */
struct snappy_hip_compress_item {
    const void *d_input;        /* 16-byte aligned device pointer */
    uint64_t input_len;         /* < 4 GiB */
    void *d_slots;              /* num_blocks(input_len) * slot_stride bytes, 16-byte aligned */
    void *d_block_bytes;        /* num_blocks(input_len) u32 */
};
SNAPPY_HIP_API int snappy_hip_compress_blocks_batch(const struct snappy_hip_compress_item *items, uint32_t count, uint32_t block_size,
                                     uint32_t slot_stride, void *d_scratch, uint64_t scratch_bytes, void *stream);

/*
 * Exclusive scan of d_block_bytes + gather of the slots into the contiguous framed stream
 * (header written too).  d_offsets: scratch/out, num_blocks+1 u64 (offset of each block in
 * d_stream; [num_blocks] = stream length, also stored to *d_stream_len if non-NULL).
 * This is the device-side form of the per-tasklet fwrite concat, snappy_compress.c:697-704.
 */
SNAPPY_HIP_API int snappy_hip_compact(const uint8_t *d_slots, uint32_t slot_stride, const uint32_t *d_block_bytes,
                       uint64_t input_len, uint32_t block_size,
                       uint8_t *d_stream, uint64_t *d_offsets, uint64_t *d_stream_len, void *stream);

/*
 * Find the u32 size chains of `count` streams from the streams' bytes alone, the device form of the
 * host pre-scan snappy_decompress.c:317-340.  d_descs: device array of `count` descriptors; for every stream
 * block_offsets[0 .. num_blocks) and result[0] (SNAPPY_HIP_BLOCK_OK / _INVALID), result[1] (blocks found) are written.
 * The chain is first sought in parallel: 256 walkers per stream start at recognised block boundaries and walk their
 * share; the shares are laid end to end iff each one ends exactly on the next one's starting point and the hops number
 * num_blocks -- which makes them the chain, whatever the recognition did.  A stream this leaves unresolved (blocks of a
 * few bytes, a damaged stream, a stream of 4 GiB or more) is walked serially, one wavefront per stream, with the same
 * result.  SNAPPY_HIP_INDEX_PARALLEL=0: the serial walk only.
 * Uses a library-owned device workspace (2.1 MB per stream of the call), allocated on first use and when a call brings
 * more streams than any before it on this device: that is the only case in which this function calls the allocator (and
 * waits for the previous call on that device); otherwise it only enqueues.
 */
SNAPPY_HIP_API int snappy_hip_index_streams(const snappy_hip_stream_desc *d_descs, uint32_t count, void *stream);

/*
 * Check candidate indexes against the size chains of `count` streams, every link in parallel: a caller that already
 * holds the block offsets -- the d_offsets array snappy_hip_compact just produced for the same stream, or an index kept
 * beside the file -- need not repeat the serial walk, but the stream stays the authority: d_descs[i].block_offsets must
 * hold num_blocks + 1 entries with [0] = header_len, [num_blocks] = stream_len, and the u32 stored at [b] leading
 * exactly to [b + 1] for every b, which is the result of the walk of snappy_decompress.c:317-340 by induction.
 * result[0] = SNAPPY_HIP_BLOCK_OK when every link holds, SNAPPY_HIP_BLOCK_INVALID otherwise (then use
 * snappy_hip_index_streams, which needs no candidate); result[1] = number of links that hold.
 */
SNAPPY_HIP_API int snappy_hip_verify_index(const snappy_hip_stream_desc *d_descs, uint32_t count, void *stream);

/*
 * K2: decode every block (semantics of snappy_decompress.c:232-285 on well-formed streams,
 * strict otherwise).  Block i is read at d_stream + d_block_offsets[i] and decoded to
 * d_out + i*block_size; d_status[i] = SNAPPY_HIP_BLOCK_*.
 */
SNAPPY_HIP_API int snappy_hip_decompress_blocks(const uint8_t *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                 uint64_t total_len, uint32_t block_size,
                                 uint8_t *d_out, uint32_t *d_status, void *stream);

/*
 * K2 over a batch of streams in ONE launch: the same per-block semantics as snappy_hip_decompress_blocks for every item
 * (its own stream, block offsets, output and status arrays; all with the same block_size), the persistent wavefronts
 * drawing blocks of all streams from one counter, so the batch has one tail instead of one per stream -- the device-side
 * form of the reference decoding many independent files, one `dpu_snappy` run each (snappy/dpu_snappy.c:186-192).  items is
 * a HOST array, empty streams are skipped, lists longer than 8 non-empty streams are issued as several launches.
 */
struct snappy_hip_decompress_item {
    const void *d_stream;          /* device: the framed stream (its header)                */
    uint64_t stream_len;           /* bytes; ignored when d_stream_len is given             */
    const void *d_stream_len;      /* device u64 or NULL: the length as left by snappy_hip_compact (*d_stream_len), so that a
                                      compress -> decompress chain needs no host round trip for it */
    const void *d_block_offsets;   /* device: num_blocks(total_len) u64                     */
    uint64_t total_len;            /* uncompressed length from the header                   */
    void *d_out;                   /* device: total_len bytes                               */
    void *d_status;                /* device: num_blocks(total_len) u32                     */
};
SNAPPY_HIP_API int snappy_hip_decompress_blocks_batch(const struct snappy_hip_decompress_item *items, uint32_t count, uint32_t block_size,
                                       void *stream);

/*
 * K2 with a whole workgroup on every block (csrc/snappy_k2_wide.hpp): for launches of a few blocks -- small files -- where
 * snappy_hip_decompress_blocks leaves most of the device idle behind one wavefront per block.  Opt-in; same arguments, same
 * answers: d_status[b] is exactly what snappy_hip_decompress_blocks writes for these arguments, where it is
 * SNAPPY_HIP_BLOCK_OK the block's output bytes are too, and nothing outside d_out[0, total_len) is written whatever the
 * stream holds.  waves_per_block wavefronts (0 = 16; else 2, 4, 8 or 16) find a block's elements in shares, prove the chain
 * with K2's own element tests and resolve the copies in LDS.  A block takes that path only within the limits -- a block_size of
 * at most SNAPPY_HIP_WIDE_MAX_BLOCK, a size word and payload inside the stream, at most SNAPPY_HIP_WIDE_MAX_CSZ
 * compressed bytes (every compressor-made block of at most 32 KiB) -- and every other block, and every block the wide path
 * does not prove, is decoded by K2's serial decoder inside the same launch: every SNAPPY_HIP_BLOCK_INVALID is its verdict.
 * A block_size above SNAPPY_HIP_WIDE_MAX_BLOCK is no error: every block goes serial.
 * d_result (4 u32, always written by an accepted call): [0] blocks the wide path decoded, [1] blocks sent to the serial
 * decoder by the limits, [2] blocks the wide path did not prove, [3] 0.
 * Only enqueues (the memsets of d_result and d_status, the work counter, one kernel on min(blocks, compute units) workgroups;
 * SNAPPY_HIP_K2_WAVES caps that number of workgroups).  total_len == 0 launches nothing and writes d_result = 0.
 * SNAPPY_HIP_ERR_ARG: a null d_result, null pointers with blocks present, a bad block_size or waves_per_block.
 */
#define SNAPPY_HIP_WIDE_MAX_BLOCK 32768u
#define SNAPPY_HIP_WIDE_MAX_CSZ   38400u   /* >= 32 + 32768 + 32768 / 6 */
SNAPPY_HIP_API int snappy_hip_decompress_blocks_wide(const uint8_t *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                      uint64_t total_len, uint32_t block_size, uint8_t *d_out, uint32_t *d_status,
                                      uint32_t waves_per_block, uint32_t *d_result, void *stream);

/*
 * Byte ranges of framed containers, decoded without the rest of them.  Range i asks for uncompressed bytes
 * [offset, offset + length) of container d_descs[stream] and gets them at dst.  Only the blocks a range touches are decoded:
 * a block wholly inside the range in place in dst, the first and last block of the range -- when only part of them is
 * wanted -- into a slot of d_scratch, from which the wanted bytes are copied to dst.
 *
 * d_descs: device array of `count` snappy_hip_stream_desc, with stream, stream_len, block_offsets (num_blocks entries, as
 *   snappy_hip_index_streams or snappy_hip_compact leave them), total_len, block_size and num_blocks filled in (result is
 *   not read).  Containers may have different block sizes, none above max_block_size.
 * d_ranges, d_status: device arrays of range_count entries, so that ranges can be produced on the device.
 * d_status[i] (written by the call):
 *   SNAPPY_HIP_BLOCK_OK             iff every block the range touches would be OK in snappy_hip_decompress_blocks (strict:
 *                                   every touched block is decoded in full, even when only part of it is wanted);
 *   SNAPPY_HIP_BLOCK_INVALID        otherwise; the contents of dst are then unspecified;
 *   SNAPPY_HIP_RANGE_OUT_OF_BOUNDS  a malformed request: stream >= count, offset + length > total_len or overflowing, a
 *                                   container whose block size is 0 or above max_block_size or whose num_blocks is too small
 *                                   for the range, a null dst with length > 0, or a range whose pieces lie beyond the
 *                                   2^31st of the call (a piece = one block of one range).  Nothing is written to its dst.
 * A range of length 0 is OK and writes nothing.  Nothing outside [dst, dst + length) of any range is ever written, whatever
 * the streams hold; ranges may overlap in their containers, not in their destinations.
 *
 * d_scratch: 256-byte aligned device workspace, not shared with a launch that runs concurrently; contents need not be
 * initialised.  It holds the ranges' piece prefix (range_count + 2 u64, rounded up to 256 bytes) and then one slot of
 * max_block_size bytes, rounded up to 256, per wavefront.  The pieces are counted on the device, so the grid is K2's for an
 * unbounded count -- one wavefront per wavefront slot of the current device, SNAPPY_HIP_K2_WAVES caps it -- or the number of
 * slots the scratch holds, whichever is smaller; a scratch too small for one slot is SNAPPY_HIP_ERR_ARG.  snappy_hip_decompress_ranges_scratch_bytes returns the size for
 * the full grid on the current device (e.g. 256 MiB + prefix for 32 KiB blocks on a whole MI355X); less only means
 * fewer wavefronts.
 * The call only enqueues work on `stream`; it never synchronises.
 */
#define SNAPPY_HIP_RANGE_OUT_OF_BOUNDS 2u
typedef struct snappy_hip_range {
	uint64_t offset;      /* first uncompressed byte of the container            */
	uint64_t length;      /* bytes                                               */
	void *dst;            /* device: length bytes, any alignment                 */
	uint32_t stream;      /* index into d_descs                                  */
	uint32_t pad;
} snappy_hip_range;
SNAPPY_HIP_API uint64_t snappy_hip_decompress_ranges_scratch_bytes(uint32_t max_block_size, uint32_t range_count);
SNAPPY_HIP_API int snappy_hip_decompress_ranges(const snappy_hip_stream_desc *d_descs, uint32_t count, const snappy_hip_range *d_ranges,
                                 uint32_t range_count, uint32_t *d_status, uint32_t max_block_size, void *d_scratch,
                                 uint64_t scratch_bytes, void *stream);

/*
 * Byte ranges of ONE framed container overwritten, recompressing only the blocks they touch.  Write i puts `length` bytes
 * from src over uncompressed bytes [offset, offset + length) of the container d_desc describes.  The blocks the writes
 * touch ("dirty") are decoded (K2's decoder), patched and compressed again (K1, LDS-table form); every other block's
 * `u32 size + elements` are copied as they are.  Blocks are independent and K1 is bit-identical to the reference per block,
 * so for a container this library, the reference or any compressor with the reference's per-block output produced,
 *     the new stream == the compressor's output for the plaintext with the writes applied, byte for byte.
 * Overwrites only: total_len, block_size and the number of blocks do not change (snappy_hip_resize below changes the length).
 *
 * d_desc: device, ONE snappy_hip_stream_desc as snappy_hip_decompress_ranges reads it (stream, stream_len, block_offsets of
 *   num_blocks entries, total_len, block_size, num_blocks; result is not read).  total_len and block_size are the host's
 *   copies of its fields: they size the launches.  A descriptor that disagrees with them is REJECTED (below).
 * d_writes, d_write_status: device arrays of write_count entries.  The writes are SORTED BY OFFSET AND DO NOT OVERLAP: write
 *   i starts at or after the end of write i - 1 (a block finds its writes by binary search).  Checked on the device.  A write
 *   of length 0 is allowed and dirties nothing.
 * d_new_stream (new_stream_capacity bytes): the header, then every block in order.  d_new_offsets (num_blocks + 1 entries,
 *   as snappy_hip_compact leaves them): [b] = offset of block b's size prefix, [num_blocks] = *d_new_stream_len = the new
 *   length.  The old stream is never written; d_new_stream must not overlap it, the sources or the scratch.
 * d_write_status[i] (always written):
 *   SNAPPY_HIP_BLOCK_OK             the write is well-formed;
 *   SNAPPY_HIP_RANGE_OUT_OF_BOUNDS  offset + length beyond total_len or overflowing, or a null src with length > 0;
 *   SNAPPY_HIP_WRITE_UNORDERED      it starts before the end of the write in front of it (the end of an overflowing write
 *                                   counts as infinite).
 * d_result[0] (always written), d_result[1] = the number of dirty blocks:
 *   SNAPPY_HIP_BLOCK_OK             done.
 *   SNAPPY_HIP_UPDATE_REJECTED      all or nothing: some write is not OK, or the writes dirty more than max_dirty_blocks
 *                                   blocks (d_result[1] = how many), or the new length exceeds new_stream_capacity, or the
 *                                   descriptor's total_len / block_size / num_blocks are not the host's.  *d_new_stream_len
 *                                   = 0 and NOT ONE BYTE of d_new_stream or d_new_offsets is written.  The later kernels read
 *                                   the verdict from device memory and leave; the host is not asked.
 *   SNAPPY_HIP_BLOCK_INVALID        the container itself is bad: a clean block whose chain link does not hold
 *                                   (offsets[b] + 4 + le32(stream + offsets[b]) == offsets[b + 1], the last one against
 *                                   stream_len: the rule of snappy_hip_verify_index, so a copy never reads outside the
 *                                   stream), or a dirty block that is only partly overwritten and does not decode under
 *                                   the strictness of snappy_hip_decompress_blocks.  *d_new_stream_len = 0; the contents of
 *                                   d_new_stream / d_new_offsets are unspecified; the old stream is intact.
 *   A dirty block that the writes cover completely (one write or several adjacent ones) is not decoded at all: its old bytes
 *   cannot matter.  A clean block is copied, NOT decoded: damage inside its payload with an intact link travels along
 *   into the new stream (snappy_hip_decompress_blocks of the new stream reports it, as it would for the old one).
 *   snappy_hip_check_blocks (below) finds such damage in the old or the new stream without decoding either.
 * No write at all gives a copy of the stream (chain checked); total_len == 0 gives the header.
 *
 * d_scratch: 256-byte aligned device workspace of at least snappy_hip_update_scratch_bytes(...) bytes for the same
 * block_size, number of blocks and max_dirty_blocks on the current device, not shared with a launch that runs
 * concurrently; contents need not be initialised.  It holds two u32 per block, two u32 and one compressed slot
 * (snappy_hip_slot_stride) per dirty block, and one patch slot (block_size + 64 bytes, rounded up to 256) per wavefront of
 * the recompress kernel: min(max_dirty_blocks, the wavefronts resident on the device with K2's stage and the LDS-table
 * kernel's table in LDS -- four per CU at 32 KiB blocks).
 * The call only enqueues work on `stream`; it never synchronises and never calls the allocator.  A second update can run on
 * the first one's outputs: d_new_stream / d_new_offsets go into the next descriptor, with an 8-byte device copy of
 * *d_new_stream_len into its stream_len.
 * SNAPPY_HIP_ERR_ARG (host side): null pointers, a bad block size, a scratch that is too small or misaligned,
 * max_dirty_blocks == 0 with writes present.
 * Rewriting beats a full recompress only while few blocks are dirty; DESIGN.md 3.5 has the measured crossover.
 */
#define SNAPPY_HIP_WRITE_UNORDERED 3u
#define SNAPPY_HIP_UPDATE_REJECTED 4u
typedef struct snappy_hip_write {
	uint64_t offset;      /* first uncompressed byte of the container that is overwritten */
	uint64_t length;      /* bytes                                               */
	const void *src;      /* device: length bytes, any alignment                 */
	uint64_t pad;
} snappy_hip_write;
SNAPPY_HIP_API uint64_t snappy_hip_update_scratch_bytes(uint32_t block_size, uint32_t num_blocks, uint32_t write_count,
                                         uint32_t max_dirty_blocks);
SNAPPY_HIP_API int snappy_hip_update_ranges(const snappy_hip_stream_desc *d_desc, uint32_t total_len, uint32_t block_size,
                             const snappy_hip_write *d_writes, uint32_t write_count, uint32_t *d_write_status,
                             uint8_t *d_new_stream, uint64_t new_stream_capacity, uint64_t *d_new_offsets,
                             uint64_t *d_new_stream_len, uint32_t *d_result, uint32_t max_dirty_blocks, void *d_scratch,
                             uint64_t scratch_bytes, void *stream);

/*
 * ONE framed container grown and shrunk in place: truncate (no segments), append (keep_len == total_len), or "rewrite from
 * here on" (both).  The new plaintext is the first keep_len bytes of the old one followed by the bytes of the segments in
 * order.  Every block wholly in front of keep_len ("kept": blocks 0 .. keep_len / block_size - 1) is copied as it is; the
 * block keep_len cuts (when keep_len % block_size != 0) is decoded (K2's decoder) and, with every block behind it up to the
 * new last one, compressed (K1, LDS-table form).  Blocks are independent and K1 is bit-identical to the reference per block,
 * so for a container this library, the reference or any compressor with the reference's per-block output produced,
 *     the new stream == the compressor's output for plaintext[0, keep_len) + the segments' bytes, byte for byte
 * -- the header has the new length (so a kept block's new offset need not be its old one) and the last block is compressed
 * at its new length (K1 sizes its hash table by it, as the reference does, snappy_compress.c:139-146).
 *
 * d_desc: device, ONE snappy_hip_stream_desc as snappy_hip_update_ranges reads it (stream, stream_len, block_offsets of
 *   num_blocks entries, total_len, block_size, num_blocks; result is not read).  total_len, block_size, keep_len and
 *   new_total_len are the host's copies: they size the launches.  The device checks that the descriptor's total_len,
 *   block_size and num_blocks are the host's, that keep_len <= total_len, and that keep_len + the sum of the segments'
 *   lengths (in 64 bits) == new_total_len.
 * d_segments, d_segment_status: device arrays of segment_count entries, so that segments can be produced on the device.  A
 *   segment of length 0 is allowed (its src may be null) and brings nothing.
 * d_new_stream (new_stream_capacity bytes): the header, then every block in order.  d_new_offsets (new_num_blocks + 1
 *   entries, new_num_blocks = snappy_hip_num_blocks(new_total_len, block_size), as snappy_hip_compact leaves them): [b] =
 *   offset of block b's size prefix, [new_num_blocks] = *d_new_stream_len = the new length.  The old stream is never written;
 *   d_new_stream must not overlap it, the sources or the scratch.
 * d_segment_status[i] (always written):
 *   SNAPPY_HIP_BLOCK_OK             the segment is well-formed;
 *   SNAPPY_HIP_RANGE_OUT_OF_BOUNDS  a null src with length > 0.
 * d_result[0] (always written):
 *   SNAPPY_HIP_BLOCK_OK             done.  d_result[1] = the number of blocks that were compressed.
 *   SNAPPY_HIP_UPDATE_REJECTED      all or nothing: some segment is not OK, or keep_len + the lengths is not new_total_len
 *                                   (a length of 2^32 or more never is), or keep_len > total_len, or the descriptor's total_len
 *                                   / block_size / num_blocks are not the host's (d_result[1] = 0 for all of these), or the new
 *                                   length exceeds new_stream_capacity (d_result[1] = the blocks that were compressed).
 *                                   *d_new_stream_len = 0 and NOT ONE BYTE of d_new_stream or d_new_offsets is written.  The
 *                                   later kernels read the verdict from device memory and leave; the host is not asked.
 *   SNAPPY_HIP_BLOCK_INVALID        the container itself is bad: a kept block whose chain link does not hold (offsets[b] + 4 +
 *                                   le32(stream + offsets[b]) == offsets[b + 1], the last one against stream_len: the rule of
 *                                   snappy_hip_verify_index, so a copy never reads outside the stream), or a cut block that
 *                                   does not decode under the strictness of snappy_hip_decompress_blocks (it is decoded in
 *                                   full, not only its first keep_len % block_size bytes).  d_result[1] = the number of
 *                                   blocks that were compressed; *d_new_stream_len = 0; the contents of d_new_stream /
 *                                   d_new_offsets are unspecified; the old stream is intact.
 *   Blocks wholly behind keep_len are never read: damage there cannot matter.  With keep_len on a block boundary nothing is
 *   decoded at all.  A kept block is copied, NOT decoded: damage inside its payload with an intact link travels along.
 *   snappy_hip_check_blocks (below) finds such damage in the old or the new stream without decoding either.
 *   keep_len == total_len without segments gives the stream again (chain checked, a short last block decoded and compressed
 *   again); new_total_len == 0 gives the header.
 *
 * d_scratch: 256-byte aligned device workspace of at least snappy_hip_resize_scratch_bytes(...) bytes for the same
 * block_size, new_total_len, keep_len and segment_count on the current device (old_num_blocks sizes nothing today), not shared
 * with a launch that runs concurrently; contents need not be initialised.  It holds one u64 per segment, two u32 per block of
 * the new container, a u32 and one compressed slot (snappy_hip_slot_stride) per compressed block, and one patch slot
 * (block_size + 64 bytes, rounded up to 256) per wavefront of the recompress kernel, as in snappy_hip_update_ranges.
 * The call only enqueues work on `stream`; it never synchronises and never calls the allocator.  A resize can follow an
 * update or another resize (and the other way round): d_new_stream / d_new_offsets go into the next descriptor, with an 8-byte
 * device copy of *d_new_stream_len into its stream_len.
 * SNAPPY_HIP_ERR_ARG (host side): null pointers, a bad block size, a scratch that is too small or misaligned.  (A new
 * length that does not fit the format's 32 bits cannot be passed: new_total_len is a uint32_t.  The drop-in call below and
 * the Python binding refuse it.)
 * The compressed blocks go through K1's LDS-table form only -- few wavefronts per CU -- as the update's dirty blocks do.  A
 * caller that appends gigabytes should compress the new data with snappy_hip_compress_blocks instead; DESIGN.md 3.7 is where
 * the measured crossover belongs.
 */
typedef struct snappy_hip_segment {
	const void *src;      /* device: length bytes, any alignment                 */
	uint64_t length;      /* bytes                                               */
} snappy_hip_segment;
SNAPPY_HIP_API uint64_t snappy_hip_resize_scratch_bytes(uint32_t block_size, uint32_t old_num_blocks, uint32_t new_total_len, uint32_t keep_len,
                                         uint32_t segment_count);
SNAPPY_HIP_API int snappy_hip_resize(const snappy_hip_stream_desc *d_desc, uint32_t total_len, uint32_t block_size,
                      uint32_t keep_len, uint32_t new_total_len,
                      const snappy_hip_segment *d_segments, uint32_t segment_count, uint32_t *d_segment_status,
                      uint8_t *d_new_stream, uint64_t new_stream_capacity, uint64_t *d_new_offsets,
                      uint64_t *d_new_stream_len, uint32_t *d_result, void *d_scratch, uint64_t scratch_bytes, void *stream);

/*
 * Containers checked without being decoded: would every block be SNAPPY_HIP_BLOCK_OK in snappy_hip_decompress_blocks?  A
 * block's verdict there depends on the stream's bytes alone -- a rejected element, output beyond the block's length, a copy
 * with a zero offset or one reaching before the block's first byte, a block that ends short of or beyond its output or its
 * compressed size, a size word that leaves the stream -- so the check walks the elements of every block as the decoder does
 * and writes nothing but verdicts: no output buffer, no stores to one, no loads of back-references.  What to run before
 * trusting a file, after a chain of snappy_hip_update_ranges / snappy_hip_resize calls (which copy clean blocks unread), or
 * as a scrub over resident containers.
 *
 * d_descs: device array of `count` snappy_hip_stream_desc as snappy_hip_decompress_ranges reads them (stream, stream_len,
 *   block_offsets of num_blocks entries, total_len, block_size, num_blocks; result is neither read nor written, so the
 *   descriptors of a snappy_hip_index_streams call can be passed on unchanged).  Containers of different block sizes mix in
 *   one call.
 * d_block_status: NULL, or a device array of `count` device pointers, any of which may be NULL.  d_block_status[i][b], when
 *   given, is exactly what snappy_hip_decompress_blocks would write to d_status[b] for that stream, those offsets and that
 *   total_len.
 * d_results: device, 4 u32 per container, always written:
 *   [4i]     SNAPPY_HIP_BLOCK_OK             every block is OK (total_len == 0: no blocks, OK);
 *            SNAPPY_HIP_BLOCK_INVALID        some block is not;
 *            SNAPPY_HIP_RANGE_OUT_OF_BOUNDS  a malformed descriptor -- block_size 0 or above 65535, num_blocks not
 *                                            ceil(total_len / block_size), null block_offsets with blocks present, a null
 *                                            stream with stream_len > 0 -- or a container whose blocks lie beyond the 2^31st
 *                                            of the call.  Nothing of it is read.
 *   [4i + 1] the number of invalid blocks;
 *   [4i + 2] the lowest invalid block index, 0xffffffff when there is none;
 *   [4i + 3] 0.
 * It checks ELEMENTS, NOT LINKS: a block is read at the offset the descriptor gives, and a block whose offset is garbage gets
 * the decoder's verdict for that offset.  A caller whose offsets are unproven runs snappy_hip_verify_index or
 * snappy_hip_index_streams first.
 * d_scratch: 256-byte aligned device workspace of at least snappy_hip_check_scratch_bytes(count) bytes (count + 2 u64, rounded
 * up to 256), not shared with a launch that runs concurrently; contents need not be initialised.  The grid is K2's
 * (SNAPPY_HIP_K2_WAVES caps it).
 * count == 0 is OK and launches nothing.  The call only enqueues work on `stream`; it never synchronises and never calls the
 * allocator.  SNAPPY_HIP_ERR_ARG (host side): null arrays with count > 0, a scratch that is too small or misaligned.
 * DESIGN.md 3.8 has the measured cost beside a decode of the same stream.
 */
SNAPPY_HIP_API uint64_t snappy_hip_check_scratch_bytes(uint32_t count);
SNAPPY_HIP_API int snappy_hip_check_blocks(const snappy_hip_stream_desc *d_descs, uint32_t count, uint32_t *const *d_block_status,
                            uint32_t *d_results, void *d_scratch, uint64_t scratch_bytes, void *stream);

/* ---- 1a. batches of raw Snappy streams, described on the device ---------- */

/*
 * The ORIGINAL ("raw") Snappy format: varint32(uncompressed length) followed by ONE element stream whose back-references may
 * reach back as far as the stream is long -- what Parquet and ORC pages, Arrow IPC buffers, RPC payloads and `snzip -t raw`
 * hold, and what every other Snappy library reads.  Many independent buffers, each described by one 32-byte item that the
 * kernels read from DEVICE memory (the host never sees the items), for both directions.
 *
 * ONE RAW STREAM IS ONE WAVEFRONT'S WORK in snappy_hip_raw_decompress_batch: element boundaries in a raw stream cannot be
 * found without parsing it, so that call does not split a stream among wavefronts the way the framed format's blocks are.
 * From this project's figure of 0.5-0.6 ms per 32 KiB block and wavefront that is an estimated 55-65 MB/s per stream (an
 * estimate, not a measurement of this kernel); the device is full only with thousands of items.  Decoding ONE large raw file
 * with that call is therefore slower than the host mode.  That is a property of that call, not of the format: streams are
 * built from independently compressed fragments, and snappy_hip_raw_decompress_split_batch (below) finds and proves them.
 * (Compression has no such limit: the fragments of one item compress in parallel.)  CHECKING one large stream has no such
 * limit either, and needs no fragments: snappy_hip_raw_check_split_batch (below) spreads any stream over the device.
 */
typedef struct snappy_hip_raw_item {
	const void *src;        /* device: the input of this item, any alignment            */
	uint64_t src_len;       /* bytes                                                    */
	void *dst;              /* device: where the output goes, any alignment             */
	uint64_t dst_capacity;  /* bytes available at dst                                   */
} snappy_hip_raw_item;
#define SNAPPY_HIP_RAW_DST_TOO_SMALL 5u
#define SNAPPY_HIP_RAW_TOO_LARGE     6u
/* The longest stream and the longest output the decoder takes: 2 GiB - 4 KiB.  Its cursors are 32 bits wide; the sum it forms
 * that grows fastest is "output so far + output of one 64-byte window" <= 2 * MAX_LEN + 1408, which must stay below 2^32
 * (csrc/snappy_raw.hpp has the whole argument). */
#define SNAPPY_HIP_RAW_MAX_LEN 0x7ffff000ull

/*
 * Item i's src[0, src_len) is one raw Snappy stream from any compressor; it is decoded to dst.  d_items, d_out_len, d_status:
 * device arrays of `count` entries.  Per item, always written: d_status[i] and d_out_len[i].
 *   SNAPPY_HIP_BLOCK_OK            dst[0, d_out_len[i]) holds the plaintext.  A stream of length 0 is OK iff nothing follows
 *                                  its header.
 *   SNAPPY_HIP_BLOCK_INVALID       src is null, or the header is malformed (a varint32 as Google's decoder reads it: at most
 *                                  5 bytes, the fifth below 16, inside src_len): d_out_len[i] = 0.  Or the elements do not
 *                                  decode under the strictness of snappy_hip_decompress_blocks: a zero offset, a reference
 *                                  before the first output byte, an element or literal payload running past src_len, output
 *                                  beyond the header's length, a stream that ends before or after the output is complete;
 *                                  the contents of dst[0, length) are then unspecified.  All four element types, offsets of
 *                                  any size, literals of any length the header allows.
 *   SNAPPY_HIP_RAW_DST_TOO_SMALL   the header's length exceeds dst_capacity (a null dst counts as capacity 0): not one byte
 *                                  written.
 *   SNAPPY_HIP_RAW_TOO_LARGE       src_len or the header's length exceeds SNAPPY_HIP_RAW_MAX_LEN: nothing written.
 * d_out_len[i] = the header's length whenever the header parses, so a first call with capacities of 0 sizes the outputs.
 * Whatever the streams hold, nothing outside [dst, dst + length) of any item is written.  The outputs must not overlap each
 * other or any source.  count == 0 is OK and launches nothing.
 * The call only enqueues work on `stream`; it never synchronises, never calls the allocator and needs no scratch.
 * SNAPPY_HIP_ERR_ARG (host side): null arrays with count > 0.
 */
SNAPPY_HIP_API int snappy_hip_raw_decompress_batch(const snappy_hip_raw_item *d_items, uint32_t count, uint64_t *d_out_len,
                                    uint32_t *d_status, void *stream);

/*
 * Item i's src[0, src_len) checked without being decoded; dst and dst_capacity are ignored.  For every item (d_status[i],
 * d_out_len[i]) equals what snappy_hip_raw_decompress_batch gives the same src and src_len with a sufficient dst_capacity:
 * SNAPPY_HIP_BLOCK_OK, SNAPPY_HIP_BLOCK_INVALID or SNAPPY_HIP_RAW_TOO_LARGE, never SNAPPY_HIP_RAW_DST_TOO_SMALL; d_out_len[i]
 * = the header's length whenever the header parses.  The payload of a long literal is skipped, not read.
 * count == 0 is OK and launches nothing.  The call only enqueues work on `stream`; it never synchronises, never calls the
 * allocator and needs no scratch.  SNAPPY_HIP_ERR_ARG (host side): null arrays with count > 0.
 * One wavefront walks a whole stream: for one LARGE stream use snappy_hip_raw_check_split_batch (below).
 */
SNAPPY_HIP_API int snappy_hip_raw_check_batch(const snappy_hip_raw_item *d_items, uint32_t count, uint64_t *d_out_len, uint32_t *d_status,
                               void *stream);

/*
 * snappy_hip_raw_decompress_batch with every LARGE item decoded by many wavefronts.  For every item (d_status[i],
 * d_out_len[i]) equals what snappy_hip_raw_decompress_batch gives the same item; when the status is SNAPPY_HIP_BLOCK_OK,
 * dst[0, length) does too; whatever the streams hold, nothing outside [dst, dst + length) is written.
 * How: streams are built from fragments -- Google's compressor, pyarrow and snappy_hip_raw_compress_batch compress fixed-size
 * pieces of the plaintext independently -- so at every multiple of the fragment size an element starts and no copy reaches
 * back across it.  The call cuts the compressed bytes into segments, walks the element chains of every segment in parallel,
 * joins them along the item (the one serial step: a table lookup per segment), finds the element that starts each UNIT of
 * unit_len output bytes, and decodes every unit with the strict decoder as a stream of its own, which refuses a copy that
 * reaches before the unit.  That last step is the proof: an item whose units all decode is byte for byte the serial decode.
 * Every other item -- not built that way, damaged, or beyond the limits below -- FALLS BACK to the serial decoder inside the
 * same call, so the result never depends on the shape of the stream, only the time does (csrc/snappy_raw_split.hpp).
 *   unit_len       output bytes per independent piece; 0 = 65,536 (what Google's compressor and pyarrow use).  At least 256.
 *                  For the output of snappy_hip_raw_compress_batch: its block_size or a multiple of it.
 *   segment_bytes  compressed bytes per segment; 0 = the default, 16 KiB (the fastest of 16 / 64 / 256 KiB measured, DESIGN.md
 *                  3.9).  A multiple of 64, at least 128.
 *   max_segments,  what the scratch has room for: the segments (ceil((src_len - header) / segment_bytes)) and the units
 *   max_units      (ceil(length / unit_len)) of the large items are counted in item order; an item whose segments or units
 *                  lie beyond either limit, and every large item behind it, is decoded serially.  That is not an error.
 * An item is LARGE when its header's length exceeds unit_len and it has more than one segment.
 * d_result, 4 words, always written: [0] items decoded by the split path, [1] items sent straight to the serial decoder
 * because they are not large, [2] large items that fell back to the serial decoder, [3] 0.  Items settled by their header
 * (a bad header, TOO_LARGE, DST_TOO_SMALL, a length of 0) are in none of them.
 * d_scratch: 256-byte aligned device workspace of at least snappy_hip_raw_decompress_split_scratch_bytes(...) bytes (0 for bad
 * parameters), not shared with a launch that runs concurrently; contents need not be initialised.  It holds two u64 and a u32
 * per item, 528 bytes per segment and a u32 per unit.
 * The call only enqueues work on `stream` (six kernels); it never synchronises and never calls the allocator; the verdicts
 * stay on the device.  SNAPPY_HIP_ERR_ARG (host side): a bad unit_len or segment_bytes, a null d_result, null arrays with
 * count > 0, a scratch that is misaligned or too small.
 */
SNAPPY_HIP_API uint64_t snappy_hip_raw_decompress_split_scratch_bytes(uint32_t count, uint32_t unit_len, uint32_t segment_bytes,
                                                       uint64_t max_segments, uint64_t max_units);
SNAPPY_HIP_API int snappy_hip_raw_decompress_split_batch(const snappy_hip_raw_item *d_items, uint32_t count, uint32_t unit_len,
                                          uint32_t segment_bytes, uint64_t max_segments, uint64_t max_units,
                                          uint64_t *d_out_len, uint32_t *d_status, uint32_t *d_result, void *d_scratch,
                                          uint64_t scratch_bytes, void *stream);

/*
 * snappy_hip_raw_check_batch with every LARGE item checked by many wavefronts, WHATEVER ITS SHAPE.  For every item
 * (d_status[i], d_out_len[i]) equals what snappy_hip_raw_check_batch gives the same item; dst and dst_capacity are ignored.
 * How: a check needs no earlier output -- every test uses an element's own fields and its absolute output position.  The
 * call cuts the compressed bytes into segments, walks the element chains of every segment in parallel and joins them along
 * the item, as snappy_hip_raw_decompress_split_batch does (the join is the one serial step: a table lookup per segment);
 * then every stretch of the true chain is walked again by a wavefront of its own with its output position known, and every
 * element on it gets the serial checker's tests: predecode's, the length bound, and a copy's offset against its absolute
 * position.  An item whose chain ends exactly at src_len with exactly the header's length and whose stretches all pass and
 * link up is OK by the serial checker's own rules.  Every other large item is judged by the serial checker inside the same
 * call, so a VALID large stream inside the limit is always proven by the parallel path, whatever built it, and only invalid
 * ones cost the serial time (csrc/snappy_raw_check_split.hpp).  There is no unit length.
 *   segment_bytes  compressed bytes per segment; 0 = the default, 16 KiB.  A multiple of 64, at least 128.
 *   max_segments   what the scratch has room for: the segments (ceil((src_len - header) / segment_bytes)) of the large items
 *                  are counted in item order; an item whose segments lie beyond the limit, and every large item behind it, is
 *                  checked serially.  That is not an error.
 * An item is LARGE when it has more than one segment.
 * d_result, 4 words, always written by an accepted call: [0] large items the parallel path proved, [1] items that are not
 * large, checked serially, [2] large items sent to the serial checker because they are beyond max_segments or were not
 * proven, [3] 0.  Items settled by their header (a bad header, TOO_LARGE, a length of 0) are in none of them.
 * d_scratch: 256-byte aligned device workspace of at least snappy_hip_raw_check_split_scratch_bytes(...) bytes (0 for a bad
 * segment_bytes), not shared with a launch that runs concurrently; contents need not be initialised.  It holds a u64 and a
 * u32 per item (the segment prefix and the flags), 64 x 8 bytes of table per segment and a 16-byte node per segment.
 * The call only enqueues work on `stream` (five kernels); it never synchronises and never calls the allocator; the verdicts
 * stay on the device.  count == 0 is OK and writes d_result = 0.  SNAPPY_HIP_ERR_ARG (host side): a bad segment_bytes, a null
 * d_result, null arrays with count > 0, a scratch that is misaligned or too small; a refused call enqueues nothing.
 */
SNAPPY_HIP_API uint64_t snappy_hip_raw_check_split_scratch_bytes(uint32_t count, uint32_t segment_bytes, uint64_t max_segments);
SNAPPY_HIP_API int snappy_hip_raw_check_split_batch(const snappy_hip_raw_item *d_items, uint32_t count, uint32_t segment_bytes,
                                     uint64_t max_segments, uint64_t *d_out_len, uint32_t *d_status, uint32_t *d_result,
                                     void *d_scratch, uint64_t scratch_bytes, void *stream);

/*
 * Item i's src[0, src_len) is plaintext; its output is varint(src_len) followed by the elements K1 produces for each
 * block_size FRAGMENT of it in order -- byte for byte tools/to_raw_snappy.py convert() of the framed stream
 * snappy_hip_compress_blocks + snappy_hip_compact give for the same bytes and block size.  A fragment is one K1 block: the
 * block_size limits of snappy_hip_compress_blocks, a hash table of its own, no reference across fragments (which is what
 * Google's compressor does with its 64 KiB fragments, so any Snappy decoder accepts the result).  The fragments of one item
 * compress in parallel.  An empty item gives the one byte 00.
 * Per item, always written:
 *   SNAPPY_HIP_BLOCK_OK            d_out_len[i] = bytes written to dst.
 *   SNAPPY_HIP_RAW_DST_TOO_SMALL   d_out_len[i] = the size it needs; not one byte of dst is written.
 *   SNAPPY_HIP_RAW_TOO_LARGE       src_len >= 4 GiB, or the item's fragments lie beyond max_fragments of the call (the scratch
 *                                  holds no more slots; the items in front of it complete).  d_out_len[i] = 0.
 *   SNAPPY_HIP_BLOCK_INVALID       a null src with src_len > 0.  d_out_len[i] = 0.
 * d_result[0] = the fragments the whole batch needs (saturated at 2^32 - 1), so that a caller can size a second call;
 * d_result[1] = the number of items that are OK.
 * snappy_hip_raw_compress_bound: a dst_capacity that always suffices for an item of src_len bytes.
 * d_scratch: 256-byte aligned device workspace of at least snappy_hip_raw_compress_scratch_bytes(block_size, count,
 * max_fragments) bytes, not shared with a launch that runs concurrently; contents need not be initialised.  It holds one
 * u64 per item and, per fragment, a u32, a u64 and one compressed slot (snappy_hip_slot_stride).
 * The call only enqueues work on `stream`; the verdicts stay on the device.
 * SNAPPY_HIP_ERR_ARG (host side): null arrays with count > 0, a bad block size, a scratch that is misaligned or too small.
 * The fragments are compressed by K1's LDS-table form (as the update's dirty blocks are); for very large batches
 * snappy_hip_raw_compress_batch_tables (below) compresses them with K1's global-table wavefronts.
 */
SNAPPY_HIP_API uint64_t snappy_hip_raw_compress_bound(uint64_t src_len, uint32_t block_size);
SNAPPY_HIP_API uint64_t snappy_hip_raw_compress_scratch_bytes(uint32_t block_size, uint32_t count, uint32_t max_fragments);
SNAPPY_HIP_API int snappy_hip_raw_compress_batch(const snappy_hip_raw_item *d_items, uint32_t count, uint32_t block_size,
                                  uint32_t max_fragments, uint64_t *d_out_len, uint32_t *d_status, uint32_t *d_result,
                                  void *d_scratch, uint64_t scratch_bytes, void *stream);

/*
 * snappy_hip_raw_compress_batch with the fragments compressed by K1's GLOBAL-table wavefronts (csrc/snappy_items_gt.hpp,
 * DESIGN.md 3.15): the table of a wavefront lives in d_tables behind a filter (and, for block sizes above 8 KiB, a slot cache)
 * in LDS, as in snappy_hip_compress_blocks, so a CU holds as many of them as it has wavefront slots where the LDS-table form
 * fits about four at 32 KiB fragments.  The same items, parameters, d_scratch (snappy_hip_raw_compress_scratch_bytes) and
 * results as the base call: every d_out_len[i], d_status[i], d_result[0], d_result[1] and every byte of every dst are
 * identical, not one byte is written outside [dst, dst + dst_capacity), a DST_TOO_SMALL item keeps all of dst.  Only the time
 * differs.
 * d_result has FOUR words here, all always written by an accepted call: [0] and [1] as in the base call, [2] = the fragments
 * that global-table wavefronts compressed, [3] = 0.
 * d_tables: the 256-byte aligned workspace snappy_hip_compress_blocks takes; snappy_hip_compress_scratch_bytes() bytes give the
 * full grid, fewer only mean fewer wavefronts (one 64 KiB table each behind a 256-byte head); room for one table is the least.
 * Contents need not be initialised; it must not be shared with a launch that runs concurrently.
 * The grid is the smallest of max_fragments, the global-table wavefronts the device holds, the tables of d_tables and
 * SNAPPY_HIP_GT_WAVES when set (read per call).  A batch of no more fragments (max_fragments) than LDS-table wavefronts are
 * resident at this block size -- the base call's grid -- runs the base call's fragment kernel, the few-blocks case being the
 * LDS form's win, and d_result[2] = 0; SNAPPY_HIP_GT_WAVES set asks for global-table wavefronts whatever the size.
 * The call only enqueues work on `stream` (one compress kernel, no helper stream); it never synchronises and never calls the
 * allocator.  Opt-in, so refused, not ignored -- SNAPPY_HIP_ERR_ARG with nothing enqueued: a null, misaligned or too small
 * d_tables, and each of the base call's own cases.
 */
SNAPPY_HIP_API int snappy_hip_raw_compress_batch_tables(const snappy_hip_raw_item *d_items, uint32_t count, uint32_t block_size,
                                         uint32_t max_fragments, uint64_t *d_out_len, uint32_t *d_status, uint32_t *d_result,
                                         void *d_scratch, uint64_t scratch_bytes, void *d_tables, uint64_t tables_bytes,
                                         void *stream);

/* ---- 1a'. the Snappy framing format (.sz) and CRC-32C on the device ------ */

/*
 * The Snappy FRAMING format: what `snzip` writes by default (.sz) and Go's snappy.Writer / Reader, snappy-java's framed streams
 * and python-snappy's stream classes speak; the one Snappy format that carries a checksum.  A stream is a chain of chunks: one
 * type byte, a 3-byte little-endian length L, L bytes.
 *   0xff        stream identifier: L = 6, "sNaPpY".  The first chunk; it may appear again anywhere (concatenated files).
 *   0x00        compressed data: the masked CRC-32C (little-endian) of the UNCOMPRESSED bytes, then one raw Snappy stream of at
 *               most 65,536 uncompressed bytes.
 *   0x01        uncompressed data: the masked CRC, then L - 4 <= 65,536 plain bytes.
 *   0x80..0xfe  padding / reserved skippable: skipped.        0x02..0x7f  reserved unskippable: the stream is refused.
 * CRC-32C: the Castagnoli polynomial (reflected 0x82F63B78), init and final xor 0xFFFFFFFF; mask(c) = ((c >> 15) | (c << 17)) +
 * 0xa282ead8.  Items are snappy_hip_raw_item (1a).
 */
typedef struct snappy_hip_crc_item {
    const uint8_t *src;    /* device pointer, any alignment; may be NULL when src_len is 0 */
    uint64_t src_len;      /* any length */
} snappy_hip_crc_item;

/*
 * d_crc[i] = the (unmasked) CRC-32C of item i's src[0, src_len); 0 for an empty item (or a null src).  d_items and d_crc are
 * device pointers to `count` entries.  One wavefront computes one item's CRC (persistent wavefronts draw items from a
 * counter), so the device is full only with many items.  The call only enqueues work on `stream`.
 */
SNAPPY_HIP_API int snappy_hip_crc32c_batch(const snappy_hip_crc_item *d_items, uint32_t count, uint32_t *d_crc, void *stream);

#define SNAPPY_HIP_SZ_CRC_MISMATCH 7u
#define SNAPPY_HIP_SZ_UNSUPPORTED  8u
#define SNAPPY_HIP_SZ_NO_VERIFY    1u   /* flags bit 0: do not compare the chunks' CRCs */

/*
 * Item i's src[0, src_len) is one .sz stream from any writer; its data chunks are decoded to dst back to back.  One wavefront
 * per stream walks the chunk chain (serial per stream), then the data chunks of the whole batch are decoded in parallel, one
 * wavefront per chunk, which also computes the CRC-32C of what it wrote and compares it with the stored one.
 * Per item, always written:
 *   SNAPPY_HIP_BLOCK_OK            dst[0, d_out_len[i]) is the plaintext, every CRC held (or flags had SNAPPY_HIP_SZ_NO_VERIFY).
 *   SNAPPY_HIP_BLOCK_INVALID       the CHAIN is broken -- a null src, no identifier, a first chunk that is not the identifier, a
 *                                  wrong identifier, a chunk running past src_len, a data chunk with L < 4 or of more than 65,536
 *                                  uncompressed bytes, an unreadable length in a compressed chunk: d_out_len[i] = 0 and not one
 *                                  byte of dst is written -- or a compressed CHUNK does not decode to the length it states: the
 *                                  other chunks are decoded, d_bad_chunk[i] names the lowest-numbered bad one.
 *   SNAPPY_HIP_SZ_UNSUPPORTED      the chain holds a reserved unskippable chunk (0x02..0x7f).  d_out_len[i] = 0, dst untouched.
 *   SNAPPY_HIP_SZ_CRC_MISMATCH     chunk d_bad_chunk[i] (the lowest-numbered bad one) decodes but its CRC does not hold.
 *   SNAPPY_HIP_RAW_DST_TOO_SMALL   the chain parses, d_out_len[i] = the total length exceeds dst_capacity (a null dst counts as
 *                                  0): not one byte of dst is written.  A first call with capacities of 0 sizes the outputs.
 *   SNAPPY_HIP_RAW_TOO_LARGE       src_len or the total length exceeds SNAPPY_HIP_RAW_MAX_LEN, or the item's chunks lie beyond
 *                                  max_chunks of the call (the items in front of it complete).
 * d_out_len[i] is the total uncompressed length whenever the chain parses.  d_bad_chunk[i]: the number, among the item's data
 * chunks, of the first one that is bad, 0xffffffff if none (also for every fault of the chain).  Nothing outside
 * [dst, dst + dst_capacity) is ever written.
 * d_result[0] = the data chunks the whole batch needs (saturated at 2^32 - 1), d_result[1] = the number of items that are OK.
 * d_scratch: 256-byte aligned device workspace of at least snappy_hip_sz_decompress_scratch_bytes(count, max_chunks) bytes
 * (a u64 per item, 32 bytes per chunk), not shared with a launch that runs concurrently; contents need not be initialised.
 * The call only enqueues work on `stream`.  SNAPPY_HIP_ERR_ARG (host side): null arrays, an unknown flag, a bad scratch.
 * There is no checksum-verifying check without an output buffer: the CRC is over the plaintext.
 */
SNAPPY_HIP_API uint64_t snappy_hip_sz_decompress_scratch_bytes(uint32_t count, uint32_t max_chunks);
SNAPPY_HIP_API int snappy_hip_sz_decompress_batch(const snappy_hip_raw_item *d_items, uint32_t count, uint32_t max_chunks, uint32_t flags,
                                   uint64_t *d_out_len, uint32_t *d_status, uint32_t *d_bad_chunk, uint32_t *d_result,
                                   void *d_scratch, uint64_t scratch_bytes, void *stream);

/*
 * snappy_hip_sz_decompress_batch with the chunk chain of every LARGE item walked by many wavefronts: for ONE large .sz file,
 * where the base call spends nearly all its time on one wavefront reading one chunk header after another.
 * CONTRACT.  Given the same items, max_chunks and flags as snappy_hip_sz_decompress_batch, the following are identical: for every
 * item d_status[i], d_out_len[i] and d_bad_chunk[i]; d_result[0] and d_result[1]; every byte of dst the base call defines.
 * Nothing outside [dst, dst + dst_capacity) is written.  A sizing call (capacities of 0) takes the parallel walk too.
 * How: the compressed bytes are cut into segments.  Segment 0 starts at offset 0; every other segment scans its share for the
 * first position that looks like a chunk start -- a type 0x00, 0x01 or 0xff header whose length and first bytes are plausible and
 * from which four more such chunks follow (or the stream ends); skippable types are never taken -- its ANCHOR.  A wavefront per
 * anchored segment applies the base call's per-chunk tests from its anchor until it lands exactly on a later segment's anchor,
 * reaches src_len, or meets a chunk the base call refuses.  A join follows these links from segment 0: the item is PROVEN iff
 * the path reaches src_len with no refusal on it.  The path's chunks are then exactly the chunks the base call's walk visits; a
 * wrongly guessed anchor is never landed on by the true chain, so it costs time and never an answer, and every large item with
 * a valid chain inside max_segments is proven.  Every other item -- not large, beyond max_segments, or not proven -- is walked by
 * one wavefront as in the base call, whose verdict is therefore the answer for every invalid chain.  The decode and the CRC
 * comparison are the base call's (csrc/snappy_sz_split.hpp).
 *   segment_bytes  compressed bytes per segment; 0 = the default, 1 MiB.  A multiple of 64, at least 256.
 *   max_segments   what the scratch has room for: the segments (ceil(src_len / segment_bytes)) of the large items are counted
 *                  in item order; an item whose segments lie beyond the limit, and every large item behind it, is walked
 *                  serially.  That is not an error.
 * An item is LARGE when src_len > segment_bytes.
 * d_result, 4 words, always written by an accepted call: [0] and [1] as in snappy_hip_sz_decompress_batch, [2] large items whose
 * chain the parallel walk proved, [3] large items walked serially (beyond max_segments, or not proven).  Items that are not
 * large, or settled before any walk (a null src, src_len above SNAPPY_HIP_RAW_MAX_LEN), are in neither.
 * d_scratch: 256-byte aligned device workspace of at least snappy_hip_sz_decompress_split_scratch_bytes(...) bytes (0 for a bad
 * segment_bytes), not shared with a launch that runs concurrently; contents need not be initialised.  It holds the base call's
 * scratch, a u64 and a u32 per item and 40 bytes per segment.
 * The call only enqueues work on `stream` (eight kernels, none of which waits on another workgroup); it never synchronises and
 * never calls the allocator.  count == 0 is OK.  SNAPPY_HIP_ERR_ARG (host side, nothing enqueued): a bad segment_bytes, an
 * unknown flag, null arrays with count > 0, a null d_result, a scratch that is misaligned or too small.
 */
SNAPPY_HIP_API uint64_t snappy_hip_sz_decompress_split_scratch_bytes(uint32_t count, uint32_t max_chunks, uint32_t segment_bytes,
                                                      uint64_t max_segments);
SNAPPY_HIP_API int snappy_hip_sz_decompress_split_batch(const snappy_hip_raw_item *d_items, uint32_t count, uint32_t max_chunks,
                                         uint32_t segment_bytes, uint64_t max_segments, uint32_t flags, uint64_t *d_out_len,
                                         uint32_t *d_status, uint32_t *d_bad_chunk, uint32_t *d_result, void *d_scratch,
                                         uint64_t scratch_bytes, void *stream);

/*
 * Item i's src[0, src_len) is plaintext; its output is the 10-byte stream identifier and one chunk per chunk_len (1..65535, K1's
 * block limits) bytes of it, in order.  With R = varint32(n) + the elements K1 produces for the chunk's n bytes as one block
 * (what snappy_hip_raw_compress_batch writes for those bytes alone), the chunk is of type 0x00 and carries R iff R is shorter
 * than n bytes, else of type 0x01 and carries the plain bytes; either way behind the masked CRC-32C of the plain bytes.  The
 * output is fully determined by the input and chunk_len; an empty item gives the identifier alone.
 * snappy_hip_sz_compress_bound = 10 + 8 * chunks + src_len: the exact size when no chunk compresses, never exceeded.
 * Statuses, d_result, d_scratch (snappy_hip_sz_compress_scratch_bytes(chunk_len, count, max_chunks)) and the host-side errors
 * are those of snappy_hip_raw_compress_batch with chunks for fragments.
 */
SNAPPY_HIP_API uint64_t snappy_hip_sz_compress_bound(uint64_t src_len, uint32_t chunk_len);
SNAPPY_HIP_API uint64_t snappy_hip_sz_compress_scratch_bytes(uint32_t chunk_len, uint32_t count, uint32_t max_chunks);
SNAPPY_HIP_API int snappy_hip_sz_compress_batch(const snappy_hip_raw_item *d_items, uint32_t count, uint32_t chunk_len, uint32_t max_chunks,
                                 uint64_t *d_out_len, uint32_t *d_status, uint32_t *d_result, void *d_scratch,
                                 uint64_t scratch_bytes, void *stream);

/*
 * snappy_hip_sz_compress_batch with the chunks compressed by K1's global-table wavefronts: what
 * snappy_hip_raw_compress_batch_tables is to snappy_hip_raw_compress_batch, with chunks for fragments -- identical outputs, a
 * d_result of four words ([2] = the chunks that global-table wavefronts compressed, [3] = 0), the same d_tables, grid,
 * small-batch rule and refusals.  The CRC, sizes and gather kernels are the base call's.
 */
SNAPPY_HIP_API int snappy_hip_sz_compress_batch_tables(const snappy_hip_raw_item *d_items, uint32_t count, uint32_t chunk_len,
                                        uint32_t max_chunks, uint64_t *d_out_len, uint32_t *d_status, uint32_t *d_result,
                                        void *d_scratch, uint64_t scratch_bytes, void *d_tables, uint64_t tables_bytes,
                                        void *stream);

/* ---- 1a''. byte ranges of .sz streams from a resident chunk index -------- */

/*
 * The data chunks of a .sz stream are as independent as a container's blocks: each holds at most 65,536 bytes of plaintext behind a
 * CRC-32C of its own.  snappy_hip_sz_index_batch walks the chains once and leaves an INDEX in the caller's memory -- one
 * snappy_hip_sz_chunk per data chunk, one snappy_hip_sz_desc per stream -- and snappy_hip_sz_decompress_ranges decodes byte ranges
 * of the plaintext from it, touching only the chunks the ranges touch (csrc/snappy_sz_ranges.hpp).
 */
typedef struct snappy_hip_sz_chunk {   /* 32 bytes: one DATA chunk of a stream */
    uint64_t src_off;   /* of the chunk's type byte in the stream                         */
    uint64_t dst_off;   /* of its first plaintext byte in the stream's plaintext           */
    uint32_t info;      /* L | bytes of the varint << 24 | (type 0x00) << 28               */
    uint32_t ulen;      /* uncompressed length, <= 65,536                                  */
    uint32_t item;      /* the item of the index call                                      */
    uint32_t reserved;  /* 0 */
} snappy_hip_sz_chunk;

typedef struct snappy_hip_sz_desc {    /* 40 bytes: one indexed stream */
    const uint8_t *src; uint64_t src_len;
    const snappy_hip_sz_chunk *chunks; uint64_t num_chunks;
    uint64_t total_len;
} snappy_hip_sz_desc;

/*
 * The index of `count` .sz streams.  The items are snappy_hip_raw_item; their dst and dst_capacity are IGNORED.  Every chain is
 * walked exactly as snappy_hip_sz_decompress_split_batch walks it (the parallel walk for items of more than segment_bytes, the
 * serial walk for the rest, the same segment_bytes / max_segments rules).  The records of all items go to d_chunks[0, max_chunks)
 * in item order; d_descs[i] = { src, src_len, d_chunks + the first chunk of item i, num_chunks, total_len }.
 * d_status[i]: what the decode call answers with unlimited capacity before any chunk is decoded -- SNAPPY_HIP_BLOCK_OK,
 * SNAPPY_HIP_BLOCK_INVALID, SNAPPY_HIP_SZ_UNSUPPORTED or SNAPPY_HIP_RAW_TOO_LARGE, never SNAPPY_HIP_RAW_DST_TOO_SMALL.  An item
 * that is not OK gets num_chunks = 0 and total_len = 0: no range can touch it.
 * d_result: 4 words with the split call's meanings; [1] counts the items indexed OK.
 * d_scratch: 256-byte aligned, at least snappy_hip_sz_index_scratch_bytes(...) bytes (0 for a bad segment_bytes): the split call's
 * scratch, a shadow item and a u64 per item.  The call only enqueues work on `stream` and never calls the allocator.
 * SNAPPY_HIP_ERR_ARG (host side, nothing enqueued): the split call's cases.
 */
SNAPPY_HIP_API uint64_t snappy_hip_sz_index_scratch_bytes(uint32_t count, uint32_t max_chunks, uint32_t segment_bytes, uint64_t max_segments);
SNAPPY_HIP_API int snappy_hip_sz_index_batch(const snappy_hip_raw_item *d_items, uint32_t count, uint32_t max_chunks, uint32_t segment_bytes,
                              uint64_t max_segments, snappy_hip_sz_chunk *d_chunks, snappy_hip_sz_desc *d_descs, uint32_t *d_status,
                              uint32_t *d_result, void *d_scratch, uint64_t scratch_bytes, void *stream);

/*
 * Range r asks for plaintext bytes [offset, offset + length) of the stream d_descs[stream] and gets them at dst.  Its PIECES are
 * the data chunks first..last of that stream: first = the largest k with dst_off[k] <= offset, last = the largest k with
 * dst_off[k] <= offset + length - 1; empty chunks between them are pieces too.  A piece wholly inside the range is decoded in
 * place, the first and last piece -- when only part of them is wanted -- into a 65,536-byte slot of d_scratch, from which the
 * wanted bytes are copied.  Unless flags has SNAPPY_HIP_SZ_NO_VERIFY the CRC-32C of every piece is compared, over the whole chunk.
 * d_status[r], always written:
 *   SNAPPY_HIP_BLOCK_OK             every touched chunk decodes to its stated length and holds its CRC;
 *   SNAPPY_HIP_BLOCK_INVALID or
 *   SNAPPY_HIP_SZ_CRC_MISMATCH      the status of the LOWEST-NUMBERED bad chunk the range touches; d_bad_chunk[r] is its number in
 *                                   its stream.  The contents of dst are then unspecified but confined to the range;
 *   SNAPPY_HIP_RANGE_OUT_OF_BOUNDS  stream >= count, offset + length > total_len or overflowing, a null dst with length > 0, a desc
 *                                   whose records hold no chunk at the range's start, or pieces beyond the 2^31st of the call.
 *                                   Nothing is written to dst.
 * d_bad_chunk[r] is 0xffffffff unless a chunk is named.  A chunk the range does not touch never influences the answer.  A range
 * of length 0 is OK and writes nothing.
 * The index is the caller's memory and may be stale, and the streams are not trusted either: before a piece is decoded its record
 * is held to the desc and the stream (src_off + 4 + L <= src_len, L >= 4 + varint bytes, ulen <= 65,536, the header re-read at
 * src_off has the record's type and L, the varint re-read there states ulen); a record that fails is BLOCK_INVALID for that piece.
 * Whatever records and streams hold, nothing outside [src, src + src_len) is read (the num_chunks records excepted) and nothing
 * outside [dst, dst + length) of a range is written (the slots excepted).
 * d_scratch: 256-byte aligned; the piece prefix (range_count + 2 u64), two u64 per range, each part rounded up to 256 bytes, then
 * one slot per wavefront.  The grid is the persistent kernels' or the slots the scratch holds, whichever is smaller; room for one
 * slot is valid, less is SNAPPY_HIP_ERR_ARG.  snappy_hip_sz_decompress_ranges_scratch_bytes returns the size for the full grid.
 * The call only enqueues work on `stream`.  SNAPPY_HIP_ERR_ARG (host side, nothing enqueued): an unknown flag, null arrays with
 * range_count > 0, a scratch that is misaligned or too small.
 */
SNAPPY_HIP_API uint64_t snappy_hip_sz_decompress_ranges_scratch_bytes(uint32_t range_count);
SNAPPY_HIP_API int snappy_hip_sz_decompress_ranges(const snappy_hip_sz_desc *d_descs, uint32_t count, const snappy_hip_range *d_ranges,
                                    uint32_t range_count, uint32_t flags, uint32_t *d_status, uint32_t *d_bad_chunk, void *d_scratch,
                                    uint64_t scratch_bytes, void *stream);

/* ---- 1b. drop-in level: one byte range of a framed file ----------------- */

/*
 * Bytes [offset, offset + length) of the framed stream in input (the whole file: input->buffer at its first byte,
 * input->length = file size).  Parses the header, walks the u32 size chain on the host only up to the last block the range
 * touches, copies only those blocks to the device, decodes them there (snappy_hip_decompress_ranges, one range, the
 * current device) and copies `length` bytes out.  output as in snappy_compress_gpu: realloc'd to `length` bytes, or used as
 * is when output->max is finite (SNAPPY_BUFFER_TOO_SMALL if length does not fit).  output->length = length on success.
 * SNAPPY_INVALID_INPUT: a malformed header or chain, offset + length beyond the uncompressed length, or a touched block that
 * does not decode (the strictness of snappy_decompress_gpu).  Fills every field of *runtime.
 */
SNAPPY_HIP_API snappy_status snappy_decompress_range_gpu(struct host_buffer_context *input, struct host_buffer_context *output,
                                          uint64_t offset, uint64_t length, struct program_runtime *runtime);

/*
 * The framed stream in input (the whole file: input->buffer at its first byte, input->length = file size) decoded to output
 * through snappy_hip_decompress_blocks_wide: for small files.  Parses the header and walks the whole u32 size chain on the
 * host (it must end exactly where the file does), one copy in, one wide launch on the current device with waves_per_block
 * (0, 2, 4, 8 or 16), one copy out.  output as in snappy_decompress_range_gpu: realloc'd to the header's length, or used as is
 * when output->max is finite (SNAPPY_BUFFER_TOO_SMALL if it does not fit); output->length = that length on success.  The same
 * statuses as snappy_decompress_gpu for the same file; SNAPPY_INVALID_INPUT also for a bad waves_per_block.  No sharding.
 * Fills every field of *runtime.
 */
SNAPPY_HIP_API snappy_status snappy_decompress_wide_gpu(struct host_buffer_context *input, struct host_buffer_context *output,
                                         uint32_t waves_per_block, struct program_runtime *runtime);

/*
 * The framed stream in input with bytes [offset, offset + patch->length) of its plaintext replaced by patch->buffer, written
 * to output (as in snappy_compress_gpu: realloc'd to the new size, or used as is when output->max is finite,
 * SNAPPY_BUFFER_TOO_SMALL if the new stream does not fit).  Parses the header and walks the whole u32 size chain on the
 * host, copies the whole stream to the current device, runs one snappy_hip_update_ranges there (only the touched blocks
 * are decoded and compressed again) and copies the new stream back.  The result is byte for byte what snappy_compress_gpu
 * gives for the patched plaintext.  SNAPPY_INVALID_INPUT: a malformed header or chain, offset + patch->length beyond the
 * uncompressed length, or a touched, partly overwritten block that does not decode.  Fills every field of *runtime.
 */
SNAPPY_HIP_API snappy_status snappy_update_range_gpu(struct host_buffer_context *input, struct host_buffer_context *patch, uint64_t offset,
                                      struct host_buffer_context *output, struct program_runtime *runtime);

/*
 * The framed stream in input with its plaintext cut to its first keep_len bytes and tail->buffer[0, tail->length) appended,
 * written to output (as in snappy_compress_gpu: realloc'd to the new size, or used as is when output->max is finite,
 * SNAPPY_BUFFER_TOO_SMALL if the new stream does not fit).  tail may be NULL or empty: a truncate.  Parses the header and
 * walks the whole u32 size chain on the host, copies the stream and the tail to the current device, runs one
 * snappy_hip_resize there (one segment; only the block keep_len cuts is decoded, only it and the blocks behind it are
 * compressed) and copies the new stream back.  The result is byte for byte what snappy_compress_gpu gives for the new
 * plaintext.  SNAPPY_INVALID_INPUT: a malformed header or chain, keep_len beyond the uncompressed length, a new length that
 * does not fit the format's 32 bits, or a cut block that does not decode.  Fills every field of *runtime.
 */
SNAPPY_HIP_API snappy_status snappy_resize_gpu(struct host_buffer_context *input, uint64_t keep_len, struct host_buffer_context *tail,
                                struct host_buffer_context *output, struct program_runtime *runtime);

/* ---- 1c. drop-in level: one buffer of the raw Snappy format -------------- */

/*
 * input (plaintext, less than 4 GiB) as ONE raw Snappy stream -- varint(length) + the elements of its block_size fragments,
 * what every other Snappy library reads -- written to output (as in snappy_compress_gpu: realloc'd to the stream's size, or
 * used as is when output->max is finite, SNAPPY_BUFFER_TOO_SMALL if it does not fit).  One item through
 * snappy_hip_raw_compress_batch on the current device; no sharding.  The bytes are tools/to_raw_snappy.py convert() of what
 * snappy_compress_gpu writes for the same input and block size.  Fills every field of *runtime.
 */
SNAPPY_HIP_API snappy_status snappy_compress_raw_gpu(struct host_buffer_context *input, struct host_buffer_context *output,
                                      uint32_t block_size, struct program_runtime *runtime);

/*
 * snappy_compress_raw_gpu through snappy_hip_raw_compress_batch_tables (1a): the same output, byte for byte; the table
 * workspace (snappy_hip_compress_scratch_bytes()) is allocated and freed by the call.
 */
SNAPPY_HIP_API snappy_status snappy_compress_raw_tables_gpu(struct host_buffer_context *input, struct host_buffer_context *output,
                                             uint32_t block_size, struct program_runtime *runtime);

/*
 * The raw Snappy stream in input (the whole file: input->buffer at its first byte, input->length = file size; from any
 * compressor) decoded to output (realloc'd to the header's length, or used as is when output->max is finite,
 * SNAPPY_BUFFER_TOO_SMALL if it does not fit).  One item through snappy_hip_raw_decompress_batch on the current device: ONE
 * wavefront decodes the whole stream, so for one large file this is slower than the host mode (see 1a).
 * SNAPPY_INVALID_INPUT: a malformed header, a stream or length above SNAPPY_HIP_RAW_MAX_LEN, or elements that do not decode.
 * Fills every field of *runtime.
 */
SNAPPY_HIP_API snappy_status snappy_decompress_raw_gpu(struct host_buffer_context *input, struct host_buffer_context *output,
                                        struct program_runtime *runtime);

/*
 * snappy_decompress_raw_gpu through snappy_hip_raw_decompress_split_batch (1a): the same file, the same output, the same
 * verdicts, but a large stream is decoded by many wavefronts where it is built from independent pieces of unit_len output
 * bytes (0 = 65,536, what Google's compressor and pyarrow write; for a file of `dpu_snappy -c -R -b N`: N or a multiple),
 * and by the serial decoder inside the same call where it is not.  One item, limits sized from the file, the default
 * segment size.  SNAPPY_INVALID_INPUT also for a unit_len between 1 and 255.  Fills every field of *runtime.
 */
SNAPPY_HIP_API snappy_status snappy_decompress_raw_split_gpu(struct host_buffer_context *input, struct host_buffer_context *output,
                                              uint32_t unit_len, struct program_runtime *runtime);

/* ---- 1c'. drop-in level: one buffer of the Snappy framing format (.sz) ---- */

/*
 * input (plaintext, less than 4 GiB) as one .sz stream of chunk_len (1..65535) chunks, written to output (as in
 * snappy_compress_gpu: realloc'd to the stream's size, or used as is when output->max is finite, SNAPPY_BUFFER_TOO_SMALL if it
 * does not fit).  One item through snappy_hip_sz_compress_batch on the current device; no sharding.  The bytes are the ones
 * `dpu_snappy -c -z` writes in host mode.  Fills every field of *runtime.
 */
SNAPPY_HIP_API snappy_status snappy_compress_sz_gpu(struct host_buffer_context *input, struct host_buffer_context *output,
                                     uint32_t chunk_len, struct program_runtime *runtime);

/*
 * snappy_compress_sz_gpu through snappy_hip_sz_compress_batch_tables (1a'): the same output, byte for byte; the table
 * workspace (snappy_hip_compress_scratch_bytes()) is allocated and freed by the call.
 */
SNAPPY_HIP_API snappy_status snappy_compress_sz_tables_gpu(struct host_buffer_context *input, struct host_buffer_context *output,
                                            uint32_t chunk_len, struct program_runtime *runtime);

/*
 * The .sz stream in input (the whole file, from any writer) decoded to output (realloc'd to the plaintext's length, or used as
 * is when output->max is finite, SNAPPY_BUFFER_TOO_SMALL if it does not fit).  The chunk chain is walked on the host to size
 * the call (a chain that does not parse is refused there), then one item goes through snappy_hip_sz_decompress_batch on the
 * current device: its chunks decode in parallel and every chunk's CRC-32C is compared, unless flags has
 * SNAPPY_HIP_SZ_NO_VERIFY.  SNAPPY_INVALID_INPUT: a broken chain, a reserved unskippable chunk, a chunk that does not decode or
 * fails its CRC (named on stderr).  Fills every field of *runtime.
 */
SNAPPY_HIP_API snappy_status snappy_decompress_sz_gpu(struct host_buffer_context *input, struct host_buffer_context *output,
                                       uint32_t flags, struct program_runtime *runtime);

/*
 * snappy_decompress_sz_gpu through snappy_hip_sz_decompress_split_batch (1a'): the same file, the same output, the same
 * statuses, the chunk chain of a large file walked by many wavefronts at the default segment, with a limit sized from the file.
 */
SNAPPY_HIP_API snappy_status snappy_decompress_sz_split_gpu(struct host_buffer_context *input, struct host_buffer_context *output,
                                             uint32_t flags, struct program_runtime *runtime);

/*
 * Bytes [offset, offset + length) of the plaintext of the .sz stream in input (the whole file).  The host walks the chunk chain
 * only up to the last chunk the range touches and copies only the touched chunks' bytes and their records (rebased to the copied
 * span) to the device; one range goes through snappy_hip_sz_decompress_ranges (1a'').  output as in snappy_decompress_range_gpu.
 * flags: SNAPPY_HIP_SZ_NO_VERIFY.  SNAPPY_INVALID_INPUT: a chain broken before the range ends, a range beyond the plaintext, or
 * a touched chunk that does not decode or fails its CRC-32C (named on stderr by its number among the stream's data chunks); a
 * chunk the range does not touch is never read.  Fills every field of *runtime.
 */
SNAPPY_HIP_API snappy_status snappy_decompress_sz_range_gpu(struct host_buffer_context *input, struct host_buffer_context *output,
                                             uint64_t offset, uint64_t length, uint32_t flags, struct program_runtime *runtime);

/* ---- 1d. drop-in level: is this file intact? ----------------------------- */

/*
 * What `gzip -t` answers, for the framed stream in input (the whole file: input->buffer at its first byte, input->length =
 * file size).  Parses the header and walks the whole u32 size chain on the host (in parallel shares where the stream is long
 * enough), copies the stream to the current device, runs one snappy_hip_check_blocks there and copies 16 bytes back: no
 * output buffer anywhere.  SNAPPY_OK iff the header, the chain (which must end exactly where the file does) and every block
 * hold; SNAPPY_INVALID_INPUT otherwise.  *report (may be NULL), always filled:
 *   blocks            the header's block count (0 when the header cannot be read);
 *   bad_blocks        blocks that do not decode; with a broken header or chain 1, and nothing is sent to the device;
 *   first_bad_block   the lowest such block, or the block whose link fails (the one whose size word is not in the file, that
 *                     ends beyond it, or -- for bytes left behind the chain -- the last one); 0 for a broken header;
 *                     UINT64_MAX when the file is intact;
 *   first_bad_offset  the file offset of that block's size word (0 for a broken header, UINT64_MAX when intact).
 * No sharding.  Fills every field of *runtime.
 */
typedef struct snappy_hip_check_report {
	uint64_t blocks, bad_blocks, first_bad_block, first_bad_offset;
} snappy_hip_check_report;
SNAPPY_HIP_API snappy_status snappy_check_gpu(struct host_buffer_context *input, snappy_hip_check_report *report,
                               struct program_runtime *runtime);

/*
 * The same for the raw Snappy stream in input: one item through snappy_hip_raw_check_batch on the current device (one
 * wavefront walks the whole stream).  *uncompressed_len (may be NULL) = the header's length, 0 when it cannot be read.
 * SNAPPY_INVALID_INPUT: a malformed header, a stream or length above SNAPPY_HIP_RAW_MAX_LEN, or elements that would not decode.
 * Fills every field of *runtime.  For one large file snappy_check_raw_split_gpu (below) is the faster call.
 */
SNAPPY_HIP_API snappy_status snappy_check_raw_gpu(struct host_buffer_context *input, uint64_t *uncompressed_len,
                                   struct program_runtime *runtime);

/*
 * snappy_check_raw_gpu through snappy_hip_raw_check_split_batch (1a): the same file, the same answers, the stream checked by
 * many wavefronts at the default segment, with a limit sized from the file.
 */
SNAPPY_HIP_API snappy_status snappy_check_raw_split_gpu(struct host_buffer_context *input, uint64_t *uncompressed_len,
                                         struct program_runtime *runtime);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPY_HIP_H_ */
