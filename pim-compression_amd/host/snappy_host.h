/*
 * snappy_host.h -- host (CPU) mode of the dpu_snappy CLI: the same four entry points the
 * reference exposes for its host path (snappy/snappy_compress.h:16-26, snappy/snappy_decompress.h:15-24).
 * This is the explicit "no -d" mode of the tool, selected by the user; it is never used as a
 * fallback for the GPU path (-d fails loudly instead).
 */
#ifndef SNAPPY_HOST_H_
#define SNAPPY_HOST_H_

#include "../../include/snappy_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

void setup_compression(struct host_buffer_context *input, struct host_buffer_context *output, struct program_runtime *runtime);
snappy_status snappy_compress_host(struct host_buffer_context *input, struct host_buffer_context *output, uint32_t block_size);
snappy_status setup_decompression(struct host_buffer_context *input, struct host_buffer_context *output, struct program_runtime *runtime);
snappy_status snappy_decompress_host(struct host_buffer_context *input, struct host_buffer_context *output);
/* dpu_snappy -r: one byte range of a whole framed file, decoding only the blocks it touches (each on its own) */
snappy_status snappy_decompress_range_host(struct host_buffer_context *input, struct host_buffer_context *output, uint64_t offset,
                                           uint64_t length);
/* dpu_snappy -w: patch over plaintext bytes [offset, offset + patch->length), recompressing only the blocks it touches */
snappy_status snappy_update_range_host(struct host_buffer_context *input, struct host_buffer_context *patch, uint64_t offset,
                                       struct host_buffer_context *output);
/* the uncompressed length in the header of a whole framed file (dpu_snappy -a alone keeps that many bytes) */
snappy_status snappy_total_len_host(const struct host_buffer_context *input, uint64_t *total_len);
/* dpu_snappy -t / -a: the first keep_len bytes of the plaintext, then tail's (tail may be NULL); only the block keep_len cuts is
 * decoded, only it and the blocks behind it are compressed */
snappy_status snappy_resize_host(struct host_buffer_context *input, uint64_t keep_len, struct host_buffer_context *tail,
                                 struct host_buffer_context *output);
/* dpu_snappy -R: the original ("raw") Snappy format, varint(length) + one element stream.  Compression writes the elements of
 * the input's block_size fragments without their size words (output from setup_compression); decompression (output from
 * setup_decompression, input->curr behind the header) takes streams of any compressor. */
snappy_status snappy_compress_raw_host(struct host_buffer_context *input, struct host_buffer_context *output, uint32_t block_size);
snappy_status snappy_decompress_raw_host(struct host_buffer_context *input, struct host_buffer_context *output);
/* dpu_snappy -T: is the whole framed file intact?  The chain is walked and every block decoded on its own into ONE scratch block;
 * the verdict is decompress_block_host's.  *report as snappy_check_gpu fills it. */
snappy_status snappy_check_host(const struct host_buffer_context *input, snappy_hip_check_report *report);
/* dpu_snappy -T -R: the same for one raw Snappy stream (decoded into a scratch buffer of the header's length) */
snappy_status snappy_check_raw_host(const struct host_buffer_context *input, uint64_t *uncompressed_len);
/* dpu_snappy -z: the Snappy framing format (.sz).  Compression writes, byte for byte, what snappy_hip_sz_compress_batch writes
 * for the same input and chunk_len (64..65535 here, as -b everywhere in host mode); decompression takes streams of any writer,
 * by the device's rules, and compares every chunk's CRC-32C unless no_verify.  Both malloc output->buffer. */
snappy_status snappy_compress_sz_host(struct host_buffer_context *input, struct host_buffer_context *output, uint32_t chunk_len);
snappy_status snappy_decompress_sz_host(struct host_buffer_context *input, struct host_buffer_context *output, int no_verify);
/* dpu_snappy -z -x: bytes [offset, offset + length) of a .sz file's plaintext; only the chunks the range touches are decoded and
 * judged, as snappy_hip_sz_decompress_ranges judges them.  mallocs output->buffer. */
snappy_status snappy_decompress_sz_range_host(struct host_buffer_context *input, struct host_buffer_context *output, uint64_t offset,
                                              uint64_t length, int no_verify);
double get_runtime(struct timeval *start, struct timeval *end);

#ifdef __cplusplus
}
#endif
#endif
