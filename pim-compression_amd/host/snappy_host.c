/*
 * snappy_host.c -- CPU mode of the dpu_snappy CLI (the tool's default when -d is absent, as in
 * the reference: snappy/dpu_snappy.c:173-183, :193-203).  Produces / consumes exactly the
 * reference's block-framed format:  varint(U) varint(BS) { u32le(size) elements }*
 * (snappy/README.md:19-33).  Behaviour follows snappy/snappy_compress.c:284-485 and
 * snappy/snappy_decompress.c:187-289; the decoder is stricter on malformed input.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>

#include "snappy_host.h"

#define TABLE_MAX 16384u          /* snappy_compress.c:16-17 */
#define HASH_MULT 0x1e35a7bdu     /* snappy_compress.c:163 */
#define TAIL_MARGIN 15u           /* snappy_compress.c:299 */

double get_runtime(struct timeval *start, struct timeval *end)   /* dpu_snappy.c:87-91 */
{
	return ((double)end->tv_sec - (double)start->tv_sec) + ((double)end->tv_usec - (double)start->tv_usec) / 1e6;
}

static uint32_t load32(const uint8_t *p)
{
	uint32_t v;
	memcpy(&v, p, 4);          /* little-endian hosts only, like the GPU */
	return v;
}

static uint8_t *varint_put(uint8_t *p, uint32_t v)
{
	for (; v > 0x7f; v >>= 7)
		*p++ = (uint8_t)(v | 0x80);
	*p++ = (uint8_t)v;
	return p;
}

static const uint8_t *varint_get(const uint8_t *p, const uint8_t *end, uint32_t *v)
{
	uint32_t acc = 0;
	for (int k = 0; k < 5 && p < end; k++) {
		uint8_t c = *p++;
		acc |= (uint32_t)(c & 0x7f) << (7 * k);
		if (c < 0x80) {
			*v = acc;
			return p;
		}
	}
	return NULL;
}

/* ---- compress ----------------------------------------------------------- */

struct sink {
	uint8_t *p;
};

static void put_literal(struct sink *s, const uint8_t *src, uint32_t len)   /* snappy_compress.c:202-225 */
{
	uint32_t n = len - 1;
	if (n < 60) {
		*s->p++ = (uint8_t)(n << 2);
	} else {
		uint8_t *tag = s->p++;
		uint32_t extra = 0;
		for (; n; n >>= 8, extra++)
			*s->p++ = (uint8_t)n;
		*tag = (uint8_t)((59 + extra) << 2);
	}
	memcpy(s->p, src, len);
	s->p += len;
}

static void put_copy(struct sink *s, uint32_t off, uint32_t len)           /* snappy_compress.c:234-272 */
{
	for (;;) {
		uint32_t piece = len;
		if (len >= 68)
			piece = 64;
		else if (len > 64)
			piece = 60;
		if (piece < 12 && off < 2048) {
			*s->p++ = (uint8_t)(1u | ((piece - 4) << 2) | ((off >> 8) << 5));
			*s->p++ = (uint8_t)off;
		} else {
			*s->p++ = (uint8_t)(2u | ((piece - 1) << 2));
			*s->p++ = (uint8_t)off;
			*s->p++ = (uint8_t)(off >> 8);
		}
		len -= piece;
		if (!len)
			return;
	}
}

static void host_compress_block(const uint8_t *b, uint32_t n, struct sink *s, uint16_t *tab)
{
	uint32_t entries = 256;                                /* snappy_compress.c:139-146 */
	while (entries < TABLE_MAX && entries < n)
		entries <<= 1;
	memset(tab, 0, entries * sizeof(*tab));
	const int shift = __builtin_clz(entries) + 1;          /* :288 */
	uint8_t *size_at = s->p;
	s->p += 4;                                             /* :291 */
	uint32_t lit = 0;                                      /* start of pending literal */

	if (n >= TAIL_MARGIN) {
		const uint32_t last = n - TAIL_MARGIN;
		uint32_t pos = 1, hcur = (load32(b + 1) * HASH_MULT) >> shift;
		for (;;) {
			uint32_t tries = 32, probe = pos, cand;
			for (;;) {                                     /* :336-348 */
				pos = probe;
				uint32_t h = hcur;
				probe = pos + (tries++ >> 5);
				if (probe > last)
					goto tail;
				hcur = (load32(b + probe) * HASH_MULT) >> shift;
				cand = tab[h];
				tab[h] = (uint16_t)pos;
				if (load32(b + pos) == load32(b + cand))
					break;
			}
			put_literal(s, b + lit, pos - lit);            /* :355 */
			for (;;) {                                     /* :370-398 */
				uint32_t from = pos, a = cand + 4, m = 4;
				pos += 4;
				while (pos + 4 <= n && load32(b + pos) == load32(b + a)) {
					pos += 4; a += 4; m += 4;
				}
				while (pos < n && b[pos] == b[a]) {
					pos++; a++; m++;
				}
				put_copy(s, from - cand, m);
				lit = pos;
				if (pos >= last)
					goto tail;
				tab[(load32(b + pos - 1) * HASH_MULT) >> shift] = (uint16_t)(pos - 1);
				uint32_t h = (load32(b + pos) * HASH_MULT) >> shift;
				cand = tab[h];
				tab[h] = (uint16_t)pos;
				if (load32(b + pos) != load32(b + cand))
					break;
			}
			pos++;                                         /* :400-401 */
			hcur = (load32(b + pos) * HASH_MULT) >> shift;
		}
	}
tail:
	if (lit < n)
		put_literal(s, b + lit, n - lit);                  /* :405-410 */
	uint32_t sz = (uint32_t)(s->p - size_at - 4);
	size_at[0] = (uint8_t)sz; size_at[1] = (uint8_t)(sz >> 8); size_at[2] = (uint8_t)(sz >> 16); size_at[3] = (uint8_t)(sz >> 24);
}

void setup_compression(struct host_buffer_context *input, struct host_buffer_context *output, struct program_runtime *runtime)
{
	struct timeval t0, t1;
	gettimeofday(&t0, NULL);
	/* The reference reserves 32 + n + n/6 (snappy_compress.c:446-447), which cannot hold the 4-byte
	 * prefixes of very small blocks; reserve for the smallest block size the CLI accepts (64) too. */
	unsigned long n = input->length;
	unsigned long cap = 64 + n + n / 6 + (n / 64 + 1) * 8;
	output->buffer = malloc(cap);
	output->curr = output->buffer;
	output->length = 0;
	gettimeofday(&t1, NULL);
	runtime->pre = get_runtime(&t0, &t1);
}

snappy_status snappy_compress_host(struct host_buffer_context *input, struct host_buffer_context *output, uint32_t block_size)
{
	if (block_size < 64 || block_size > 65535 || input->length > 0xffffffffUL)
		return SNAPPY_INVALID_INPUT;
	uint16_t *tab = malloc(TABLE_MAX * sizeof(*tab));
	struct sink s = { output->buffer };
	s.p = varint_put(s.p, (uint32_t)input->length);       /* :461-465 */
	s.p = varint_put(s.p, block_size);
	const uint8_t *in = input->buffer;
	unsigned long left = input->length;
	while (left) {                                        /* :467-479 */
		uint32_t n = left < block_size ? (uint32_t)left : block_size;
		host_compress_block(in, n, &s, tab);
		in += n;
		left -= n;
	}
	free(tab);
	input->curr = input->buffer + input->length;
	output->curr = s.p;
	output->length = (unsigned long)(s.p - output->buffer);
	return SNAPPY_OK;
}

/* ---- decompress ---------------------------------------------------------- */

snappy_status setup_decompression(struct host_buffer_context *input, struct host_buffer_context *output, struct program_runtime *runtime)
{
	struct timeval t0, t1;
	gettimeofday(&t0, NULL);
	uint32_t total;
	const uint8_t *p = varint_get(input->curr, input->buffer + input->length, &total);   /* :193-198 */
	if (!p) {
		fprintf(stderr, "Failed to read decompressed length\n");
		return SNAPPY_INVALID_INPUT;
	}
	input->curr = (uint8_t *)p;
	if (total > output->max) {                            /* :200-204 */
		fprintf(stderr, "Output length is to big: max=%ld len=%d\n", output->max, total);
		return SNAPPY_BUFFER_TOO_SMALL;
	}
	output->buffer = malloc((((unsigned long)total + 7) & ~7UL) | 2047);   /* :207 */
	output->curr = output->buffer;
	output->length = total;
	gettimeofday(&t1, NULL);
	runtime->pre = get_runtime(&t0, &t1);
	return SNAPPY_OK;
}

/* The elements of one block (snappy_decompress.c:232-285): ip .. bend decoded to op; back-references may reach down to
 * out0, output may grow up to out_end.  Returns the new output position, NULL if the block is malformed. */
static uint8_t *decompress_block_host(const uint8_t *ip, const uint8_t *bend, uint8_t *const out0, uint8_t *op, uint8_t *const out_end)
{
	while (ip < bend) {                               /* :232-285 */
		uint32_t tag = *ip++, len, off;
		if ((tag & 3) == 0) {
			len = (tag >> 2) + 1;
			if (len > 60) {
				uint32_t nb = len - 60;
				if ((uint32_t)(bend - ip) < nb)
					return NULL;
				len = 0;
				for (uint32_t k = 0; k < nb; k++)
					len |= (uint32_t)ip[k] << (8 * k);
				len += 1;
				ip += nb;
			}
			if (len == 0 || (unsigned long)(bend - ip) < len || (unsigned long)(out_end - op) < len)
				return NULL;
			memcpy(op, ip, len);
			ip += len;
			op += len;
			continue;
		}
		uint32_t need = (tag & 3) == 1 ? 1 : ((tag & 3) == 2 ? 2 : 4);
		if ((uint32_t)(bend - ip) < need)
			return NULL;
		if ((tag & 3) == 1) {
			len = ((tag >> 2) & 7) + 4;
			off = ((tag >> 5) << 8) | ip[0];
		} else if ((tag & 3) == 2) {
			len = (tag >> 2) + 1;
			off = ip[0] | ((uint32_t)ip[1] << 8);
		} else {
			len = (tag >> 2) + 1;
			off = load32(ip);
		}
		ip += need;
		if (off == 0 || (unsigned long)(op - out0) < off) {
			printf("bad offset!\n");                    /* :171 */
			return NULL;
		}
		if ((unsigned long)(out_end - op) < len)
			return NULL;
		for (const uint8_t *from = op - off; len; len--)
			*op++ = *from++;
	}
	return op;
}

snappy_status snappy_decompress_host(struct host_buffer_context *input, struct host_buffer_context *output)
{
	const uint8_t *end = input->buffer + input->length;
	uint32_t bs;
	const uint8_t *ip = varint_get(input->curr, end, &bs);   /* :220-225 */
	if (!ip) {
		fprintf(stderr, "Failed to read decompressed block size\n");
		return SNAPPY_INVALID_INPUT;
	}
	uint8_t *const out0 = output->buffer;
	uint8_t *const out_end = out0 + output->length;
	uint8_t *op = out0;
	while (ip < end) {                                    /* :227-231 */
		if (end - ip < 4)
			return SNAPPY_INVALID_INPUT;
		uint32_t csz = load32(ip);
		ip += 4;
		if ((unsigned long)(end - ip) < csz)
			return SNAPPY_INVALID_INPUT;
		const uint8_t *bend = ip + csz;
		op = decompress_block_host(ip, bend, out0, op, out_end);
		if (!op)
			return SNAPPY_INVALID_INPUT;
		ip = bend;
	}
	input->curr = (uint8_t *)ip;
	output->curr = op;
	return (op == out_end) ? SNAPPY_OK : SNAPPY_INVALID_INPUT;
}

/* ---- the raw format (dpu_snappy -R) ---------------------------------------- */

/* varint(length), then the elements of every block_size fragment as host_compress_block writes them, less the size word:
 * fragments never refer to each other, so their concatenation is one valid raw stream. */
snappy_status snappy_compress_raw_host(struct host_buffer_context *input, struct host_buffer_context *output, uint32_t block_size)
{
	if (block_size < 64 || block_size > 65535 || input->length > 0xffffffffUL)
		return SNAPPY_INVALID_INPUT;
	uint16_t *tab = malloc(TABLE_MAX * sizeof(*tab));
	struct sink s = { output->buffer };
	s.p = varint_put(s.p, (uint32_t)input->length);
	const uint8_t *in = input->buffer;
	unsigned long left = input->length;
	while (left) {
		uint32_t n = left < block_size ? (uint32_t)left : block_size;
		uint8_t *const size_at = s.p;
		host_compress_block(in, n, &s, tab);
		s.p -= 4;
		memmove(size_at, size_at + 4, (size_t)(s.p - size_at));
		in += n;
		left -= n;
	}
	free(tab);
	input->curr = input->buffer + input->length;
	output->curr = s.p;
	output->length = (unsigned long)(s.p - output->buffer);
	return SNAPPY_OK;
}

/* The whole file behind its header is ONE "block": decompress_block_host's lengths, offsets and bounds are as wide as the
 * file.  The header is a varint32 as Google's decoder reads it: the fifth byte, if there is one, below 16. */
snappy_status snappy_decompress_raw_host(struct host_buffer_context *input, struct host_buffer_context *output)
{
	if (input->curr - input->buffer == 5 && input->curr[-1] >= 16)
		return SNAPPY_INVALID_INPUT;
	uint8_t *const out0 = output->buffer;
	uint8_t *const out_end = out0 + output->length;
	uint8_t *op = decompress_block_host(input->curr, input->buffer + input->length, out0, out0, out_end);
	if (!op)
		return SNAPPY_INVALID_INPUT;
	input->curr = input->buffer + input->length;
	output->curr = op;
	return (op == out_end) ? SNAPPY_OK : SNAPPY_INVALID_INPUT;
}

/* ---- the Snappy framing format (dpu_snappy -z) -------------------------------- */

/* CRC-32C (Castagnoli, reflected 0x82F63B78, init and final xor 0xffffffff) by a byte table made on first use */
static uint32_t crc32c_host(const uint8_t *p, unsigned long n)
{
	static uint32_t table[256];
	if (!table[1])
		for (uint32_t b = 0; b < 256; b++) {
			uint32_t c = b;
			for (int k = 0; k < 8; k++)
				c = (c >> 1) ^ (0x82F63B78u & (0u - (c & 1u)));
			table[b] = c;
		}
	uint32_t c = 0xffffffffu;
	while (n--)
		c = (c >> 8) ^ table[(c ^ *p++) & 0xff];
	return ~c;
}

static uint32_t crc_mask_host(uint32_t c)
{
	return ((c >> 15) | (c << 17)) + 0xa282ead8u;
}

static void put32(uint8_t *p, uint32_t v)
{
	p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

/* The bytes snappy_hip_sz_compress_batch writes: the identifier, then per chunk_len bytes one chunk -- type 0x00 with
 * varint(n) + host_compress_block's elements iff those are shorter than the n plain bytes, else type 0x01 with the plain
 * bytes -- behind the masked CRC-32C of the plain bytes.  output->buffer is malloc'd here (the exact bound). */
snappy_status snappy_compress_sz_host(struct host_buffer_context *input, struct host_buffer_context *output, uint32_t chunk_len)
{
	if (chunk_len < 64 || chunk_len > 65535 || input->length > 0xffffffffUL)
		return SNAPPY_INVALID_INPUT;
	const unsigned long chunks = (input->length + chunk_len - 1) / chunk_len;
	const unsigned long cap = 10 + 8 * chunks + input->length;
	uint16_t *tab = malloc(TABLE_MAX * sizeof(*tab));
	uint8_t *slot = malloc(4 + 32 + (unsigned long)chunk_len + chunk_len / 6 + 8);
	output->buffer = malloc(cap);
	if (!tab || !slot || !output->buffer) {
		free(tab);
		free(slot);
		return SNAPPY_BUFFER_TOO_SMALL;
	}
	uint8_t *op = output->buffer;
	memcpy(op, "\xff\x06\x00\x00sNaPpY", 10);
	op += 10;
	const uint8_t *in = input->buffer;
	unsigned long left = input->length;
	while (left) {
		const uint32_t n = left < chunk_len ? (uint32_t)left : chunk_len;
		struct sink s = { slot };
		host_compress_block(in, n, &s, tab);
		const uint32_t elements = (uint32_t)(s.p - slot) - 4;
		uint8_t var[5];
		const uint32_t vlen = (uint32_t)(varint_put(var, n) - var);
		const int compressed = vlen + elements < n;
		const uint32_t L = 4 + (compressed ? vlen + elements : n);
		put32(op, (uint32_t)(compressed ? 0x00 : 0x01) | (L << 8));
		put32(op + 4, crc_mask_host(crc32c_host(in, n)));
		if (compressed) {
			memcpy(op + 8, var, vlen);
			memcpy(op + 8 + vlen, slot + 4, elements);
		} else {
			memcpy(op + 8, in, n);
		}
		op += 4 + L;
		in += n;
		left -= n;
	}
	free(tab);
	free(slot);
	input->curr = input->buffer + input->length;
	output->curr = op;
	output->length = (unsigned long)(op - output->buffer);
	return SNAPPY_OK;
}

/* The chunk at buf + at (at < len) by the rules of snappy_hip_sz_decompress_batch: its type, its L and, for a data chunk, its
 * uncompressed length n; *identified follows the chain.  Or why the stream is refused.  Reads nothing outside [buf, buf + len). */
static snappy_status sz_chunk_host(const uint8_t *buf, unsigned long len, unsigned long at, int *identified, uint32_t *type_out,
                                   uint32_t *L_out, uint32_t *n_out)
{
	if (len - at < 4) {
		fprintf(stderr, "a chunk header runs past the end of the file\n");
		return SNAPPY_INVALID_INPUT;
	}
	const uint32_t type = buf[at], L = buf[at + 1] | (uint32_t)buf[at + 2] << 8 | (uint32_t)buf[at + 3] << 16;
	if (len - at - 4 < L) {
		fprintf(stderr, "the chunk at offset %lu runs past the end of the file\n", at);
		return SNAPPY_INVALID_INPUT;
	}
	const uint8_t *body = buf + at + 4;
	uint32_t n = 0;
	if (type == 0xff) {
		if (L != 6 || memcmp(body, "sNaPpY", 6) != 0) {
			fprintf(stderr, "a wrong stream identifier at offset %lu\n", at);
			return SNAPPY_INVALID_INPUT;
		}
		*identified = 1;
	} else if (!*identified) {
		fprintf(stderr, "the first chunk is not the stream identifier\n");
		return SNAPPY_INVALID_INPUT;
	} else if (type <= 1) {
		n = L - 4;
		if (L < 4) {
			fprintf(stderr, "the data chunk at offset %lu has no room for its checksum\n", at);
			return SNAPPY_INVALID_INPUT;
		}
		if (type == 0) {
			const uint8_t *p = varint_get(body + 4, body + L, &n);
			if (!p || (p - (body + 4) == 5 && p[-1] >= 16)) {
				fprintf(stderr, "the compressed chunk at offset %lu has no readable length\n", at);
				return SNAPPY_INVALID_INPUT;
			}
		}
		if (n > 65536) {
			fprintf(stderr, "the chunk at offset %lu holds more than 65536 bytes\n", at);
			return SNAPPY_INVALID_INPUT;
		}
	} else if (type < 0x80) {
		fprintf(stderr, "reserved unskippable chunk 0x%02x at offset %lu\n", type, at);
		return SNAPPY_INVALID_INPUT;
	}
	*type_out = type;
	*L_out = L;
	*n_out = n;
	return SNAPPY_OK;
}

/* The chunk chain of a whole .sz file: the sum of the data chunks' uncompressed lengths, or why the stream is refused. */
static snappy_status sz_walk_host(const uint8_t *buf, unsigned long len, uint64_t *total)
{
	unsigned long at = 0;
	int identified = 0;
	*total = 0;
	while (at < len) {
		uint32_t type, L, n;
		if (sz_chunk_host(buf, len, at, &identified, &type, &L, &n) != SNAPPY_OK)
			return SNAPPY_INVALID_INPUT;
		*total += n;
		at += 4ul + L;
	}
	if (!identified) {
		fprintf(stderr, "no stream identifier\n");
		return SNAPPY_INVALID_INPUT;
	}
	return SNAPPY_OK;
}

/* A whole .sz file (input->buffer at its first byte) decoded into output->buffer, malloc'd here; every chunk's CRC compared
 * unless no_verify.  A chain that does not parse, a chunk that does not decode to its stated length or fails its CRC:
 * SNAPPY_INVALID_INPUT, no output. */
snappy_status snappy_decompress_sz_host(struct host_buffer_context *input, struct host_buffer_context *output, int no_verify)
{
	const uint8_t *buf = input->buffer;
	const unsigned long len = input->length;
	uint64_t total;
	output->buffer = NULL;
	output->length = 0;
	if (sz_walk_host(buf, len, &total) != SNAPPY_OK)
		return SNAPPY_INVALID_INPUT;
	if (total > output->max)
		return SNAPPY_BUFFER_TOO_SMALL;
	uint8_t *out = malloc(total ? total : 1);
	if (!out)
		return SNAPPY_BUFFER_TOO_SMALL;
	uint8_t *op = out;
	unsigned long at = 0, k = 0;
	while (at < len) {                                     /* (the walk above has checked every bound used here) */
		const uint32_t type = buf[at], L = buf[at + 1] | (uint32_t)buf[at + 2] << 8 | (uint32_t)buf[at + 3] << 16;
		const uint8_t *body = buf + at + 4;
		if (type <= 1) {
			uint32_t n = L - 4;
			if (type == 0) {
				const uint8_t *ip = varint_get(body + 4, body + L, &n);
				if (decompress_block_host(ip, body + L, op, op, op + n) != op + n) {
					fprintf(stderr, "data chunk %lu at offset %lu does not decode\n", k, at);
					free(out);
					return SNAPPY_INVALID_INPUT;
				}
			} else {
				memcpy(op, body + 4, n);
			}
			if (!no_verify && crc_mask_host(crc32c_host(op, n)) != load32(body)) {
				fprintf(stderr, "data chunk %lu at offset %lu fails its CRC-32C\n", k, at);
				free(out);
				return SNAPPY_INVALID_INPUT;
			}
			op += n;
			k++;
		}
		at += 4ul + L;
	}
	input->curr = input->buffer + len;
	output->buffer = out;
	output->curr = op;
	output->length = (unsigned long)total;
	return SNAPPY_OK;
}

/* Bytes [offset, offset + length) of the plaintext of a .sz file, by the rules of snappy_hip_sz_decompress_ranges: the chain is
 * walked only up to the last chunk the range touches, and only the touched chunks -- chunk k with dst_off[k] <= offset + length - 1
 * and dst_off[k] + n[k] > offset, which are the device's first..last -- are decoded, in full, and their CRCs compared unless
 * no_verify.  A chain broken before the range ends, a range beyond the plaintext, a touched chunk that does not decode or fails
 * its CRC (named on stderr): SNAPPY_INVALID_INPUT, no output.  A bad chunk the range does not touch is never looked at. */
snappy_status snappy_decompress_sz_range_host(struct host_buffer_context *input, struct host_buffer_context *output, uint64_t offset,
                                              uint64_t length, int no_verify)
{
	const uint8_t *buf = input->buffer;
	const unsigned long len = input->length;
	const uint64_t end = offset + length;
	output->buffer = NULL;
	output->length = 0;
	if (end < offset) {
		fprintf(stderr, "the range [%llu, +%llu) overflows\n", (unsigned long long)offset, (unsigned long long)length);
		return SNAPPY_INVALID_INPUT;
	}
	if (length > output->max)
		return SNAPPY_BUFFER_TOO_SMALL;
	uint8_t *out = malloc(length ? length : 1), *piece = malloc(65536);
	snappy_status st = (out && piece) ? SNAPPY_OK : SNAPPY_BUFFER_TOO_SMALL;
	unsigned long at = 0, k = 0;
	uint64_t total = 0;                                      /* the plaintext in front of the chunk at `at` */
	int identified = 0;
	while (st == SNAPPY_OK && at < len && !(identified && total >= end)) {
		uint32_t type, L, n;
		if ((st = sz_chunk_host(buf, len, at, &identified, &type, &L, &n)) != SNAPPY_OK)
			break;
		if (type <= 1) {
			const uint8_t *body = buf + at + 4;
			if (length && total < end && total + n > offset) {               /* touched */
				if (type == 0) {
					uint32_t stated;
					const uint8_t *ip = varint_get(body + 4, body + L, &stated);
					if (decompress_block_host(ip, body + L, piece, piece, piece + n) != piece + n) {
						fprintf(stderr, "data chunk %lu at offset %lu does not decode\n", k, at);
						st = SNAPPY_INVALID_INPUT;
						break;
					}
				} else {
					memcpy(piece, body + 4, n);
				}
				if (!no_verify && crc_mask_host(crc32c_host(piece, n)) != load32(body)) {
					fprintf(stderr, "data chunk %lu at offset %lu fails its CRC-32C\n", k, at);
					st = SNAPPY_INVALID_INPUT;
					break;
				}
				const uint64_t from = offset > total ? offset : total, to = end < total + n ? end : total + n;
				memcpy(out + (from - offset), piece + (from - total), to - from);
			}
			total += n;
			k++;
		}
		at += 4ul + L;
	}
	if (st == SNAPPY_OK && !identified) {
		fprintf(stderr, "no stream identifier\n");
		st = SNAPPY_INVALID_INPUT;
	}
	if (st == SNAPPY_OK && total < end) {
		fprintf(stderr, "the range [%llu, %llu) lies beyond the plaintext of %llu bytes\n", (unsigned long long)offset, (unsigned long long)end,
		        (unsigned long long)total);
		st = SNAPPY_INVALID_INPUT;
	}
	free(piece);
	if (st != SNAPPY_OK) {
		free(out);
		return st;
	}
	output->buffer = out;
	output->curr = out + length;
	output->length = (unsigned long)length;
	return SNAPPY_OK;
}

/* ---- the check (dpu_snappy -T) ---------------------------------------------- */

snappy_status snappy_check_host(const struct host_buffer_context *input, snappy_hip_check_report *report)
{
	const uint8_t *const end = input->buffer + input->length;
	uint32_t total, bs;
	report->blocks = 0;
	report->bad_blocks = 1;
	report->first_bad_block = 0;
	report->first_bad_offset = 0;
	const uint8_t *ip = varint_get(input->buffer, end, &total);
	if (ip)
		ip = varint_get(ip, end, &bs);
	if (!ip) {
		fprintf(stderr, "Failed to read the stream header\n");
		return SNAPPY_INVALID_INPUT;
	}
	if (total && (bs == 0 || bs > 65535)) {
		fprintf(stderr, "block size %u in the stream is outside 1..65535\n", bs);
		return SNAPPY_INVALID_INPUT;
	}
	const uint64_t nb = total ? ((uint64_t)total + bs - 1) / bs : 0;
	report->blocks = nb;
	uint8_t *scratch = malloc(total ? bs : 1);
	if (!scratch)
		return SNAPPY_BUFFER_TOO_SMALL;
	uint64_t bad = 0, first = UINT64_MAX, first_at = UINT64_MAX, last_at = 0, b;
	int chain = 1;
	for (b = 0; b < nb; b++) {                           /* the chain (:227-231), every block on its own */
		const uint64_t at = (uint64_t)(ip - input->buffer);
		uint32_t csz = 0;
		if (end - ip >= 4)
			csz = load32(ip);
		if (end - ip < 4 || (unsigned long)(end - ip - 4) < csz) {
			chain = 0;
			first = b;
			first_at = at;
			break;
		}
		ip += 4;
		last_at = at;
		const uint64_t blen = (b + 1) * (uint64_t)bs < total ? bs : total - b * (uint64_t)bs;
		if (decompress_block_host(ip, ip + csz, scratch, scratch, scratch + blen) != scratch + blen) {
			if (!bad) {
				first = b;
				first_at = at;
			}
			bad++;
		}
		ip += csz;
	}
	free(scratch);
	if (chain && ip != end) {                            /* bytes behind the last block: its link does not reach the end */
		chain = 0;
		first = nb ? nb - 1 : 0;
		first_at = nb ? last_at : (uint64_t)(ip - input->buffer);
	}
	if (!chain) {
		fprintf(stderr, "the size chain breaks at block %lu of %lu\n", (unsigned long)first, (unsigned long)nb);
		report->bad_blocks = 1;
	} else {
		report->bad_blocks = bad;
	}
	report->first_bad_block = first;
	report->first_bad_offset = first_at;
	return (chain && !bad) ? SNAPPY_OK : SNAPPY_INVALID_INPUT;
}

snappy_status snappy_check_raw_host(const struct host_buffer_context *input, uint64_t *uncompressed_len)
{
	const uint8_t *const end = input->buffer + input->length;
	uint32_t total;
	*uncompressed_len = 0;
	const uint8_t *ip = varint_get(input->buffer, end, &total);
	if (!ip || (ip - input->buffer == 5 && ip[-1] >= 16)) {
		fprintf(stderr, "Failed to read decompressed length\n");
		return SNAPPY_INVALID_INPUT;
	}
	*uncompressed_len = total;
	uint8_t *scratch = malloc(total ? total : 1);
	if (!scratch)
		return SNAPPY_BUFFER_TOO_SMALL;
	const uint8_t *op = decompress_block_host(ip, end, scratch, scratch, scratch + total);
	const int ok = op == scratch + total;
	free(scratch);
	return ok ? SNAPPY_OK : SNAPPY_INVALID_INPUT;
}

/* Bytes [offset, offset + length) of a whole framed file (input->buffer at its first byte): the size chain walked up to the
 * last block the range touches, only the touched blocks decoded.  output->buffer is malloc'd here (length bytes). */
snappy_status snappy_decompress_range_host(struct host_buffer_context *input, struct host_buffer_context *output, uint64_t offset,
                                           uint64_t length)
{
	const uint8_t *const end = input->buffer + input->length;
	uint32_t total, bs;
	const uint8_t *ip = varint_get(input->buffer, end, &total);
	if (ip)
		ip = varint_get(ip, end, &bs);
	if (!ip) {
		fprintf(stderr, "Failed to read the stream header\n");
		return SNAPPY_INVALID_INPUT;
	}
	if (offset + length < offset || offset + length > total) {
		fprintf(stderr, "range %lu:%lu lies beyond the %u uncompressed bytes\n", (unsigned long)offset, (unsigned long)length, total);
		return SNAPPY_INVALID_INPUT;
	}
	output->buffer = malloc(length ? length : 1);
	if (!output->buffer)
		return SNAPPY_BUFFER_TOO_SMALL;
	output->curr = output->buffer;
	output->length = length;
	if (length == 0)
		return SNAPPY_OK;
	if (bs == 0)
		return SNAPPY_INVALID_INPUT;
	const uint64_t first = offset / bs, last = (offset + length - 1) / bs;
	const uint64_t lo = first * bs, hi = (last + 1) * (uint64_t)bs < total ? (last + 1) * (uint64_t)bs : total;
	uint8_t *tmp = malloc(hi - lo);
	if (!tmp)
		return SNAPPY_BUFFER_TOO_SMALL;
	snappy_status st = SNAPPY_OK;
	for (uint64_t b = 0; b <= last && st == SNAPPY_OK; b++) {       /* the chain (:227-231) up to the last touched block */
		if (end - ip < 4) {
			st = SNAPPY_INVALID_INPUT;
			break;
		}
		const uint32_t csz = load32(ip);
		ip += 4;
		if ((unsigned long)(end - ip) < csz) {
			st = SNAPPY_INVALID_INPUT;
			break;
		}
		if (b >= first) {            /* a touched block: exactly its own bytes, at its own place */
			uint8_t *const bout = tmp + (b * bs - lo);
			const uint64_t blen = (b + 1) * (uint64_t)bs < total ? bs : total - b * (uint64_t)bs;
			if (decompress_block_host(ip, ip + csz, bout, bout, bout + blen) != bout + blen)
				st = SNAPPY_INVALID_INPUT;
		}
		ip += csz;
	}
	if (st == SNAPPY_OK)
		memcpy(output->buffer, tmp + (offset - lo), length);
	free(tmp);
	return st;
}

/* dpu_snappy -w: `patch` over plaintext bytes [offset, offset + patch->length) of a whole framed file.  The chain is walked
 * once; a block the patch touches is decoded (unless the patch covers it completely), patched and compressed again, every
 * other block's size prefix and elements are copied.  output->buffer is malloc'd here. */
snappy_status snappy_update_range_host(struct host_buffer_context *input, struct host_buffer_context *patch, uint64_t offset,
                                       struct host_buffer_context *output)
{
	const uint8_t *const end = input->buffer + input->length;
	const uint64_t length = patch->length;
	uint32_t total, bs;
	const uint8_t *ip = varint_get(input->buffer, end, &total);
	if (ip)
		ip = varint_get(ip, end, &bs);
	if (!ip) {
		fprintf(stderr, "Failed to read the stream header\n");
		return SNAPPY_INVALID_INPUT;
	}
	if (offset + length < offset || offset + length > total) {
		fprintf(stderr, "write %lu:%lu lies beyond the %u uncompressed bytes\n", (unsigned long)offset, (unsigned long)length, total);
		return SNAPPY_INVALID_INPUT;
	}
	if (total && (bs == 0 || bs > 65535))
		return SNAPPY_INVALID_INPUT;
	const uint64_t nb = total ? ((uint64_t)total + bs - 1) / bs : 0;
	const uint64_t first = length ? offset / bs : 1, last = length ? (offset + length - 1) / bs : 0;   /* first > last: no dirty block */
	const uint64_t dirty = length ? last - first + 1 : 0;
	const unsigned long cap = input->length + dirty * (4ul + 32 + bs + bs / 6) + 16;
	uint8_t *out = malloc(cap), *tmp = malloc((unsigned long)bs + 16);
	uint16_t *tab = malloc(TABLE_MAX * sizeof(*tab));
	snappy_status st = (out && tmp && tab) ? SNAPPY_OK : SNAPPY_BUFFER_TOO_SMALL;
	struct sink s = { out };
	if (st == SNAPPY_OK) {
		memcpy(out, input->buffer, (size_t)(ip - input->buffer));      /* the header stays */
		s.p = out + (ip - input->buffer);
	}
	for (uint64_t b = 0; b < nb && st == SNAPPY_OK; b++) {
		if (end - ip < 4) {
			st = SNAPPY_INVALID_INPUT;
			break;
		}
		const uint32_t csz = load32(ip);
		if ((unsigned long)(end - ip - 4) < csz) {
			st = SNAPPY_INVALID_INPUT;
			break;
		}
		if (b < first || b > last) {
			memcpy(s.p, ip, 4ul + csz);
			s.p += 4ul + csz;
		} else {
			const uint64_t begin = b * bs, blen = begin + bs < total ? bs : total - begin;
			const uint64_t from = offset > begin ? offset : begin, to = offset + length < begin + blen ? offset + length : begin + blen;
			if (to - from < blen && decompress_block_host(ip + 4, ip + 4 + csz, tmp, tmp, tmp + blen) != tmp + blen) {
				st = SNAPPY_INVALID_INPUT;
				break;
			}
			memcpy(tmp + (from - begin), patch->buffer + (from - offset), to - from);
			host_compress_block(tmp, (uint32_t)blen, &s, tab);
		}
		ip += 4ul + csz;
	}
	if (st == SNAPPY_OK && ip != end)
		st = SNAPPY_INVALID_INPUT;                             /* bytes behind the last block */
	free(tmp);
	free(tab);
	if (st != SNAPPY_OK) {
		free(out);
		return st;
	}
	output->buffer = out;
	output->curr = s.p;
	output->length = (unsigned long)(s.p - out);
	return SNAPPY_OK;
}

/* The uncompressed length in the header of a whole framed file (dpu_snappy -a alone keeps that many bytes). */
snappy_status snappy_total_len_host(const struct host_buffer_context *input, uint64_t *total_len)
{
	uint32_t total;
	if (!varint_get(input->buffer, input->buffer + input->length, &total)) {
		fprintf(stderr, "Failed to read the stream header\n");
		return SNAPPY_INVALID_INPUT;
	}
	*total_len = total;
	return SNAPPY_OK;
}

/* dpu_snappy -t / -a: the first keep_len bytes of the plaintext of a whole framed file, then tail's bytes (tail may be NULL).
 * The chain is walked once, to its end; the blocks wholly in front of keep_len are copied, the block keep_len cuts is decoded
 * (in full, unless keep_len lies on a block boundary) and, with every block behind it up to the new last one, compressed; the
 * header gets the new length.  output->buffer is malloc'd here. */
snappy_status snappy_resize_host(struct host_buffer_context *input, uint64_t keep_len, struct host_buffer_context *tail,
                                 struct host_buffer_context *output)
{
	const uint8_t *const end = input->buffer + input->length;
	const uint64_t length = tail ? tail->length : 0;
	uint32_t total, bs;
	const uint8_t *ip = varint_get(input->buffer, end, &total);
	if (ip)
		ip = varint_get(ip, end, &bs);
	if (!ip) {
		fprintf(stderr, "Failed to read the stream header\n");
		return SNAPPY_INVALID_INPUT;
	}
	if (keep_len > total) {
		fprintf(stderr, "keep length %lu lies beyond the %u uncompressed bytes\n", (unsigned long)keep_len, total);
		return SNAPPY_INVALID_INPUT;
	}
	if (length > 0xffffffffUL - keep_len) {
		fprintf(stderr, "%lu + %lu bytes do not fit the format's 32-bit length\n", (unsigned long)keep_len, (unsigned long)length);
		return SNAPPY_INVALID_INPUT;
	}
	if (bs == 0 || bs > 65535 || (length && !tail->buffer))
		return SNAPPY_INVALID_INPUT;
	const uint64_t nb = ((uint64_t)total + bs - 1) / bs;
	const uint64_t new_total = keep_len + length, new_nb = (new_total + bs - 1) / bs, kept = keep_len / bs;
	/* the chain (:227-231): where the kept blocks end (= where the cut block starts), and that it ends with the file */
	const uint8_t *const first = ip, *cut = ip;
	for (uint64_t b = 0; b < nb; b++) {
		if (end - ip < 4)
			return SNAPPY_INVALID_INPUT;
		const uint32_t csz = load32(ip);
		if ((unsigned long)(end - ip - 4) < csz)
			return SNAPPY_INVALID_INPUT;
		ip += 4ul + csz;
		if (b + 1 == kept)
			cut = ip;
	}
	if (ip != end)
		return SNAPPY_INVALID_INPUT;                           /* bytes behind the last block */
	const unsigned long cap = 16 + (unsigned long)(cut - first) + (new_nb - kept) * (4ul + 32 + bs + bs / 6);
	uint8_t *out = malloc(cap), *tmp = malloc((unsigned long)bs + 16);
	uint16_t *tab = malloc(TABLE_MAX * sizeof(*tab));
	snappy_status st = (out && tmp && tab) ? SNAPPY_OK : SNAPPY_BUFFER_TOO_SMALL;
	struct sink s = { out };
	if (st == SNAPPY_OK) {
		s.p = varint_put(s.p, (uint32_t)new_total);          /* the header changes length with the new total */
		s.p = varint_put(s.p, bs);
		memcpy(s.p, first, (size_t)(cut - first));
		s.p += cut - first;
	}
	for (uint64_t b = kept; b < new_nb && st == SNAPPY_OK; b++) {
		const uint64_t begin = b * bs, n = begin + bs < new_total ? bs : new_total - begin;
		const uint64_t head = b == kept ? keep_len - begin : 0;
		if (head) {
			const uint64_t blen = begin + bs < total ? bs : total - begin;
			const uint32_t csz = load32(cut);
			if (decompress_block_host(cut + 4, cut + 4 + csz, tmp, tmp, tmp + blen) != tmp + blen) {
				st = SNAPPY_INVALID_INPUT;
				break;
			}
		}
		if (n > head)
			memcpy(tmp + head, tail->buffer + (begin + head - keep_len), n - head);
		host_compress_block(tmp, (uint32_t)n, &s, tab);
	}
	free(tmp);
	free(tab);
	if (st != SNAPPY_OK) {
		free(out);
		return st;
	}
	output->buffer = out;
	output->curr = s.p;
	output->length = (unsigned long)(s.p - out);
	return SNAPPY_OK;
}
