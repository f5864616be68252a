/*
 * dpu_snappy -- the reference's command line tool (snappy/dpu_snappy.c) re-authored for MI355X:
 * identical flags and stdout lines, `-d` now means "offload to the GPU(s)" through libsnappy_hip.so
 * (snappy_compress_gpu / snappy_decompress_gpu) where the reference called snappy_compress_dpu /
 * snappy_decompress_dpu (dpu_snappy.c:169-172, :189-192).  Without -d the host CPU codec runs,
 * as in the reference.  -d never falls back to the CPU.
 *
 *   dpu_snappy [-d] [-c] [-R] [-S [<unit_len>]] [-W [<waves>]] [-b <block_size>] [-g <gpus>] [-r <offset>:<length>] [-w <offset>:<patch_file>] [-t <keep_len>] [-a <tail_file>] -i <input_file> [-o <output_file>]
 *   dpu_snappy [-d] [-R [-S]] -T -i <input_file>
 *   dpu_snappy [-d] [-c] -z [-S] [-b <chunk_len>] -i <input_file> [-o <output_file>]
 *   dpu_snappy [-d] -z [-S] -T -i <input_file>
 *   dpu_snappy [-d] -z -x <offset>:<length> -i <input_file> [-o <output_file>]
 */
#include <getopt.h>
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>

#include "snappy_host.h"

static void usage(const char *exe)                          /* dpu_snappy.c:70-82 */
{
#ifdef DEBUG
	fprintf(stderr, "**DEBUG BUILD**\n");
#endif
	fprintf(stderr, "Compress or decompress a file with Snappy\nCan use either the host CPU or MI355X GPUs\n");
	fprintf(stderr, "usage: %s [-d] [-c] [-R] [-S [<unit_len>]] [-W [<waves>]] [-b <block_size>] [-g <gpus>] [-r <offset>:<length>] [-w <offset>:<patch_file>] [-t <keep_len>] [-a <tail_file>] -i <input_file> [-o <output_file>]\n", exe);
	fprintf(stderr, "       %s -d -c -R|-z -G [-b <block_size>] -i <input_file> [-o <output_file>]\n", exe);
	fprintf(stderr, "       %s [-d] [-R [-S]] -T -i <input_file>\n", exe);
	fprintf(stderr, "       %s [-d] [-c] -z [-S] [-b <chunk_len>] -i <input_file> [-o <output_file>]\n", exe);
	fprintf(stderr, "       %s [-d] -z [-S] -T -i <input_file>\n", exe);
	fprintf(stderr, "       %s [-d] -z -x <offset>:<length> -i <input_file> [-o <output_file>]\n", exe);
	fprintf(stderr, "d: use the GPU(s), by default host is used\n");
	fprintf(stderr, "c: perform compression, by default performs decompression\n");
	fprintf(stderr, "R: the original (raw) Snappy format, varint(length) + one element stream, instead of the block-framed one\n");
	fprintf(stderr, "z: the Snappy framing format (.sz, what snzip and the stream classes of other Snappy libraries write): chunks of <block_size> bytes, each with the CRC-32C of its plain bytes, which decompression compares; with -T: decode the file, compare every CRC, write nothing\n");
	fprintf(stderr, "G: with -d -c and -R or -z: compress the fragments (chunks) with the global-table wavefronts of the block-framed compressor; the file written is the one without -G\n");
	fprintf(stderr, "S: with -d -R, decompressing: decode one large raw stream with many wavefronts, in independent pieces of <unit_len> output bytes (default 65536; for a file of -c -R -b N: N or a multiple); a stream not built that way is decoded as without -S; with -d -R -T (no <unit_len>): check one large raw stream with many wavefronts, whatever built it; with -d -z (no <unit_len>), decompressing or with -T: walk the chunk chain of one large .sz stream with many wavefronts\n");
	fprintf(stderr, "W: with -d, decompressing a block-framed file: put a workgroup of <waves> wavefronts (2, 4, 8 or 16, default 16) on every block instead of one wavefront; for small files\n");
	fprintf(stderr, "b: block size used for compression, default is 32KB, ignored for decompression\n");
	fprintf(stderr, "g: number of GPUs to shard blocks over with -d, default all visible\n");
	fprintf(stderr, "r: decompress only <length> bytes from uncompressed byte <offset> of the input\n");
	fprintf(stderr, "x: with -z: extract only <length> bytes from plaintext byte <offset> of a .sz stream; only the chunks the range touches are read, decoded and held to their CRCs\n");
	fprintf(stderr, "w: overwrite the uncompressed bytes from <offset> with <patch_file>, recompressing only the touched blocks\n");
	fprintf(stderr, "t: keep only the first <keep_len> uncompressed bytes of the input (with -a: then append)\n");
	fprintf(stderr, "a: append <tail_file> to the uncompressed bytes, compressing only the blocks from the cut on; alone it keeps everything\n");
	fprintf(stderr, "T: test the compressed input: would every block (with -R: the raw stream) decode?  Writes no output; exit status 1 if not\n");
	fprintf(stderr, "i: input file\n");
	fprintf(stderr, "o: output file\n");
}

/* In -d mode the file buffers are page-locked (snappy_hip_host_alloc) so that the copies inside
 * snappy_*_gpu run at PCIe rate instead of through the driver's pageable bounce buffers. */
static int g_pinned = 0;

static uint8_t *buffer_alloc(unsigned long bytes)
{
	if (g_pinned) {
		uint8_t *p = snappy_hip_host_alloc(bytes);
		if (p)
			return p;
		g_pinned = 0;                /* no device: -d will fail loudly later; keep going with malloc */
	}
	return malloc(bytes ? bytes : 8);
}

static int slurp(const char *path, struct host_buffer_context *in)    /* dpu_snappy.c:23-50 */
{
	FILE *f = fopen(path, "rb");
	if (!f) {
		fprintf(stderr, "Invalid input file: %s\n", path);
		return 1;
	}
	fseek(f, 0, SEEK_END);
	long sz = ftell(f);
	rewind(f);
	if (sz < 0 || (unsigned long)sz > in->max) {
		fprintf(stderr, "input_size is too big (%ld > %ld)\n", sz, in->max);
		fclose(f);
		return 1;
	}
	in->length = (unsigned long)sz;
	in->buffer = buffer_alloc(((unsigned long)sz + 7) & ~7UL);
	in->curr = in->buffer;
	size_t got = fread(in->buffer, 1, in->length, f);
	fclose(f);
#ifdef DEBUG
	printf("%s: read %ld bytes from %s (%lu)\n", __func__, in->length, path, got);
#endif
	return got != in->length;
}

static int spill(const char *path, const struct host_buffer_context *out)   /* dpu_snappy.c:58-63 */
{
	FILE *f = fopen(path, "wb");
	if (!f) {
		fprintf(stderr, "Cannot open output file: %s\n", path);
		return 1;
	}
	size_t put = fwrite(out->buffer, 1, out->length, f);
	fclose(f);
	return put != out->length;
}

int main(int argc, char **argv)
{
	int use_gpu = 0, compress = 0, opt;
	int block_size = 32 * 1024;                              /* dpu_snappy.c:100 */
	const char *in_path = NULL, *out_path = NULL;
	struct host_buffer_context input = { 0 }, output = { 0 };
	input.max = ULONG_MAX;
	output.max = ULONG_MAX;

	int use_range = 0;
	unsigned long long range_off = 0, range_len = 0;
	int use_extract = 0;                                     /* -z -x: a range of a .sz stream's plaintext */
	unsigned long long extract_off = 0, extract_len = 0;
	int use_write = 0;
	unsigned long long write_off = 0;
	const char *patch_path = NULL;
	int raw = 0;
	int sz = 0;
	int use_keep = 0;
	unsigned long long keep_len = 0;
	const char *tail_path = NULL;
	int use_check = 0;
	int use_split = 0;
	unsigned long split_unit = 0;
	int split_has_unit = 0;
	int use_wide = 0;
	unsigned long wide_waves = 0;
	int use_tables = 0;
	while ((opt = getopt(argc, argv, "dcRzGTS::W::b:g:i:o:r:w:t:a:x:")) != -1) {
		switch (opt) {
		case 'S': {                  /* -S, -S<unit_len> or -S <unit_len> */
			const char *arg = optarg;
			if (!arg && optind < argc && argv[optind][0] >= '0' && argv[optind][0] <= '9')
				arg = argv[optind++];
			if (arg) {
				char *rest = NULL;
				split_unit = strtoul(arg, &rest, 10);
				if (rest == arg || *rest != '\0' || split_unit < 256 || split_unit > 0xffffffffUL) {
					fprintf(stderr, "-S wants <unit_len> in bytes, at least 256, got '%s'\n", arg);
					return -2;
				}
				split_has_unit = 1;
			}
			use_split = 1;
			break;
		}
		case 'W': {                  /* -W, -W<waves> or -W <waves> */
			const char *arg = optarg;
			if (!arg && optind < argc && argv[optind][0] >= '0' && argv[optind][0] <= '9')
				arg = argv[optind++];
			if (arg) {
				char *rest = NULL;
				wide_waves = strtoul(arg, &rest, 10);
				if (rest == arg || *rest != '\0' || (wide_waves != 2 && wide_waves != 4 && wide_waves != 8 && wide_waves != 16)) {
					fprintf(stderr, "-W wants <waves> per block: 2, 4, 8 or 16, got '%s'\n", arg);
					return -2;
				}
			}
			use_wide = 1;
			break;
		}
		case 'T': use_check = 1; break;
		case 't': {                  /* keep only the first keep_len uncompressed bytes */
			char *rest = NULL;
			keep_len = strtoull(optarg, &rest, 10);
			if (rest == optarg || *rest != '\0' || optarg[0] == '-' || optarg[0] == '+' || optarg[0] == ' ') {
				fprintf(stderr, "-t wants <keep_len> in bytes, got '%s'\n", optarg);
				return -2;
			}
			use_keep = 1;
			break;
		}
		case 'a': tail_path = optarg; break;
		case 'w': {                  /* overwrite the uncompressed bytes from offset with the patch file's */
			char *colon = NULL;
			write_off = strtoull(optarg, &colon, 10);
			if (colon == optarg || *colon != ':' || optarg[0] == '-' || colon[1] == '\0') {
				fprintf(stderr, "-w wants <offset>:<patch_file>, got '%s'\n", optarg);
				return -2;
			}
			patch_path = colon + 1;
			use_write = 1;
			break;
		}
		case 'r': {                  /* decompress only bytes [offset, offset + length) of the container */
			char *colon = NULL, *tail = NULL;
			range_off = strtoull(optarg, &colon, 10);
			if (colon == optarg || *colon != ':' || optarg[0] == '-' || colon[1] == '-' || colon[1] == '\0') {
				fprintf(stderr, "-r wants <offset>:<length> in bytes, got '%s'\n", optarg);
				return -2;
			}
			range_len = strtoull(colon + 1, &tail, 10);
			if (*tail != '\0') {
				fprintf(stderr, "-r wants <offset>:<length> in bytes, got '%s'\n", optarg);
				return -2;
			}
			use_range = 1;
			break;
		}
		case 'x': {                  /* extract only bytes [offset, offset + length) of a .sz stream's plaintext */
			char *colon = NULL, *tail = NULL;
			extract_off = strtoull(optarg, &colon, 10);
			if (colon == optarg || *colon != ':' || optarg[0] == '-' || colon[1] == '-' || colon[1] == '\0') {
				fprintf(stderr, "-x wants <offset>:<length> in bytes, got '%s'\n", optarg);
				return -2;
			}
			extract_len = strtoull(colon + 1, &tail, 10);
			if (*tail != '\0') {
				fprintf(stderr, "-x wants <offset>:<length> in bytes, got '%s'\n", optarg);
				return -2;
			}
			use_extract = 1;
			break;
		}
		case 'd': use_gpu = 1; break;
		case 'c': compress = 1; break;
		case 'R': raw = 1; break;
		case 'z': sz = 1; break;
		case 'G': use_tables = 1; break;
		case 'b': block_size = atoi(optarg); break;
		case 'g': setenv("SNAPPY_HIP_NUM_GPUS", optarg, 1); break;
		case 'i': in_path = optarg; break;
		case 'o': out_path = optarg; break;
		default:
			usage(argv[0]);
			return -2;
		}
	}
	if (!in_path) {
		usage(argv[0]);
		return -1;
	}
	if (use_tables && (!use_gpu || !compress || (!raw && !sz))) {
		fprintf(stderr, "-G compresses one raw Snappy or .sz stream with global-table wavefronts: it goes with -d -c and one of -R and -z\n");
		return -2;
	}
	if (use_range && compress) {
		fprintf(stderr, "-r selects a range of a compressed file: it does not go with -c\n");
		return -2;
	}
	if (use_write && (compress || use_range)) {
		fprintf(stderr, "-w overwrites bytes of a compressed file: it does not go with -c or -r\n");
		return -2;
	}
	if (raw && (use_range || use_write)) {
		fprintf(stderr, "-R reads and writes one raw Snappy stream: it has no blocks for -r or -w to select\n");
		return -2;
	}
	if (use_extract && (!sz || compress || use_check || raw || use_split || use_wide)) {
		fprintf(stderr, "-x extracts a byte range of one .sz stream: it goes with -z and not with -c, -T, -R, -S or -W\n");
		return -2;
	}
	if (sz && (raw || use_range || use_write || use_wide || use_keep || tail_path)) {
		fprintf(stderr, "-z reads and writes one .sz stream: it goes with -c, -b, -d, -S, -T and -x only\n");
		return -2;
	}
	if (sz && use_split && split_has_unit) {
		fprintf(stderr, "-S takes no <unit_len> with -z: the chunks of a .sz stream are its units\n");
		return -2;
	}
	if (use_split && ((!raw && !sz) || compress)) {
		fprintf(stderr, "-S splits the decoding or the check (-T) of one raw Snappy or .sz stream: it goes with -R or -z and not with -c\n");
		return -2;
	}
	if (use_split && use_check && split_has_unit) {
		fprintf(stderr, "-S takes no <unit_len> with -T: a check has no units\n");
		return -2;
	}
	const int use_resize = use_keep || tail_path;
	if (use_wide && (compress || raw || use_range || use_write || use_resize || use_check)) {
		fprintf(stderr, "-W decodes a whole block-framed file: it does not go with -c, -R, -r, -w, -t, -a or -T\n");
		return -2;
	}
	if (use_resize && (compress || use_range || use_write || raw)) {
		fprintf(stderr, "-t and -a resize a compressed file: they do not go with -c, -r, -w or -R\n");
		return -2;
	}
	if (use_check && (compress || use_range || use_write || use_resize || out_path)) {
		fprintf(stderr, "-T tests a compressed file and writes nothing: it does not go with -c, -r, -w, -t, -a or -o\n");
		return -2;
	}
	if (use_gpu) {
		/* the overlapped copy-in / kernel / copy-out pipeline of the library keeps six HIP streams busy; HIP maps
		 * streams onto GPU_MAX_HW_QUEUES hardware queues (default 4).  The host program owns its environment, so it
		 * is set here (before the first HIP call), not by the library. */
		setenv("GPU_MAX_HW_QUEUES", "8", 0);
		/* the format's length field is a uint32 (snappy_compress.c:461); HBM is not the limit */
		input.max = 0xffffffffUL;
		output.max = 0xffffffffUL;
	}
	input.file_name = in_path;
	printf("Using input file %s\n", in_path);
	if (!out_path)
		out_path = "output.txt";                             /* dpu_snappy.c:155-157 */
	output.file_name = out_path;
	if (!use_check)
		printf("Using output file %s\n", out_path);

	g_pinned = use_gpu;
	if (slurp(in_path, &input))
		return -1;

	struct program_runtime rt;
	memset(&rt, 0, sizeof(rt));                              /* the reference leaves this uninitialised */
	snappy_status st;
	struct timeval t0, t1;
	if (sz && use_check) {
		/* the CRCs are over the plaintext: the file is decoded (into a buffer that is dropped), every CRC compared */
		output.buffer = NULL;
		output.curr = NULL;
		output.max = ULONG_MAX;
		if (use_gpu) {
			st = use_split ? snappy_decompress_sz_split_gpu(&input, &output, 0, &rt) : snappy_decompress_sz_gpu(&input, &output, 0, &rt);
		} else {                         /* (host mode ignores -S) */
			gettimeofday(&t0, NULL);
			st = snappy_decompress_sz_host(&input, &output, 0);
			gettimeofday(&t1, NULL);
			rt.run = get_runtime(&t0, &t1);
		}
		if (st == SNAPPY_BUFFER_TOO_SMALL) {
			fprintf(stderr, "Encountered Snappy error %u\n", st);
			return -1;
		}
		if (st == SNAPPY_OK)
			printf("Check: OK, %lu bytes\n", (unsigned long)output.length);
		else
			printf("Check: INVALID\n");
		printf("Pre-processing time: %f\n", rt.pre);
		printf("Alloc time: %f\n", rt.d_alloc);
		printf("Load time: %f\n", rt.load);
		printf("Copy in time: %f\n", rt.copy_in);
		printf("Host time: %f\n", rt.run);
		printf("Copy out time: %f\n", rt.copy_out);
		printf("Free time: %f\n", rt.d_free);
		return st == SNAPPY_OK ? 0 : 1;
	}
	if (use_check) {
		/* nothing is decoded to anywhere: the verdict, one line, the exit status */
		snappy_hip_check_report rep = { 0, 0, 0, 0 };
		uint64_t raw_len = 0;
		if (use_gpu) {
			st = !raw ? snappy_check_gpu(&input, &rep, &rt)
			     : use_split ? snappy_check_raw_split_gpu(&input, &raw_len, &rt)
			     : snappy_check_raw_gpu(&input, &raw_len, &rt);
		} else {
			gettimeofday(&t0, NULL);
			st = raw ? snappy_check_raw_host(&input, &raw_len) : snappy_check_host(&input, &rep);
			gettimeofday(&t1, NULL);
			rt.run = get_runtime(&t0, &t1);
		}
		if (st == SNAPPY_BUFFER_TOO_SMALL) {
			fprintf(stderr, "Encountered Snappy error %u\n", st);
			return -1;
		}
		if (raw && st == SNAPPY_OK)
			printf("Check: OK, %lu bytes\n", (unsigned long)raw_len);
		else if (raw)
			printf("Check: INVALID\n");
		else if (st == SNAPPY_OK)
			printf("Check: OK, %lu blocks\n", (unsigned long)rep.blocks);
		else
			printf("Check: INVALID, %lu of %lu blocks, first bad block %lu at offset %lu\n", (unsigned long)rep.bad_blocks,
			       (unsigned long)rep.blocks, (unsigned long)rep.first_bad_block, (unsigned long)rep.first_bad_offset);
		printf("Pre-processing time: %f\n", rt.pre);
		printf("Alloc time: %f\n", rt.d_alloc);
		printf("Load time: %f\n", rt.load);
		printf("Copy in time: %f\n", rt.copy_in);
		printf("Host time: %f\n", rt.run);
		printf("Copy out time: %f\n", rt.copy_out);
		printf("Free time: %f\n", rt.d_free);
		return st == SNAPPY_OK ? 0 : 1;
	}
	if (sz && use_extract) {
		/* only the chunks the range touches are read and decoded; both modes allocate the output */
		output.buffer = NULL;
		output.curr = NULL;
		output.max = ULONG_MAX;
		if (use_gpu) {
			st = snappy_decompress_sz_range_gpu(&input, &output, extract_off, extract_len, 0, &rt);
		} else {
			gettimeofday(&t0, NULL);
			st = snappy_decompress_sz_range_host(&input, &output, extract_off, extract_len, 0);
			gettimeofday(&t1, NULL);
			rt.run = get_runtime(&t0, &t1);
		}
	} else if (sz) {
		/* one .sz stream, either way; both modes allocate the output */
		output.buffer = NULL;
		output.curr = NULL;
		output.max = ULONG_MAX;
		if (use_gpu) {
			st = use_tables  ? snappy_compress_sz_tables_gpu(&input, &output, (uint32_t)block_size, &rt)
			     : compress  ? snappy_compress_sz_gpu(&input, &output, (uint32_t)block_size, &rt)
			     : use_split ? snappy_decompress_sz_split_gpu(&input, &output, 0, &rt)
			                 : snappy_decompress_sz_gpu(&input, &output, 0, &rt);   /* (host mode ignores -S) */
		} else {
			gettimeofday(&t0, NULL);
			st = compress ? snappy_compress_sz_host(&input, &output, (uint32_t)block_size) : snappy_decompress_sz_host(&input, &output, 0);
			gettimeofday(&t1, NULL);
			rt.run = get_runtime(&t0, &t1);
		}
	} else if (raw) {
		/* one raw Snappy stream, either way; in -d mode one item through the batch calls of the library, which allocates
		 * the output */
		if (use_gpu) {
			output.buffer = NULL;
			output.curr = NULL;
			output.max = ULONG_MAX;
			st = use_tables  ? snappy_compress_raw_tables_gpu(&input, &output, (uint32_t)block_size, &rt)
			     : compress  ? snappy_compress_raw_gpu(&input, &output, (uint32_t)block_size, &rt)
			     : use_split ? snappy_decompress_raw_split_gpu(&input, &output, (uint32_t)split_unit, &rt)
			                 : snappy_decompress_raw_gpu(&input, &output, &rt);   /* (host mode ignores -S) */
		} else {
			if (compress)
				setup_compression(&input, &output, &rt);
			else if (setup_decompression(&input, &output, &rt))
				return -1;
			gettimeofday(&t0, NULL);
			st = compress ? snappy_compress_raw_host(&input, &output, (uint32_t)block_size) : snappy_decompress_raw_host(&input, &output);
			gettimeofday(&t1, NULL);
			rt.run = get_runtime(&t0, &t1);
		}
	} else if (compress) {
		if (use_gpu && g_pinned && block_size >= 1 && block_size <= 65535) {
			/* page-locked output of the stream's upper bound; max = capacity tells the library not to realloc */
			struct timeval a, b;
			gettimeofday(&a, NULL);
			output.max = snappy_hip_stream_bound(input.length, (uint32_t)block_size);
			output.buffer = buffer_alloc(output.max);
			output.curr = output.buffer;
			gettimeofday(&b, NULL);
			rt.pre = get_runtime(&a, &b);
		} else if (use_gpu) {
			/* no page-locked memory (or an out-of-range -b, which the library rejects): the library allocates the
			 * output itself; setup_compression's 32+n+n/6 is too small for tiny block sizes (snappy_compress.c:446-449) */
			output.buffer = NULL;
			output.curr = NULL;
			output.max = ULONG_MAX;
		} else {
			setup_compression(&input, &output, &rt);
		}
		if (use_gpu) {
			st = snappy_compress_gpu(&input, &output, (uint32_t)block_size, &rt);
		} else {
			gettimeofday(&t0, NULL);
			st = snappy_compress_host(&input, &output, (uint32_t)block_size);
			gettimeofday(&t1, NULL);
			rt.run = get_runtime(&t0, &t1);
		}
	} else if (use_write) {
		/* only the blocks the patch touches are decoded and compressed again; the output is the new stream */
		struct host_buffer_context patch = { 0 };
		patch.max = ULONG_MAX;
		patch.file_name = patch_path;
		if (slurp(patch_path, &patch))
			return -1;
		output.buffer = NULL;
		output.curr = NULL;
		output.max = ULONG_MAX;
		if (use_gpu) {
			st = snappy_update_range_gpu(&input, &patch, write_off, &output, &rt);
		} else {
			gettimeofday(&t0, NULL);
			st = snappy_update_range_host(&input, &patch, write_off, &output);
			gettimeofday(&t1, NULL);
			rt.run = get_runtime(&t0, &t1);
		}
	} else if (use_resize) {
		/* only the block keep_len cuts is decoded, only it and the blocks behind it are compressed; the output is the new stream */
		struct host_buffer_context tail = { 0 };
		tail.max = ULONG_MAX;
		tail.file_name = tail_path;
		if (tail_path && slurp(tail_path, &tail))
			return -1;
		const int tail_pinned = tail_path && g_pinned;   /* (buffer_alloc clears g_pinned when it falls back to malloc) */
		if (!use_keep) {                 /* -a alone keeps everything */
			uint64_t total = 0;
			if (snappy_total_len_host(&input, &total) != SNAPPY_OK)
				return -1;
			keep_len = total;
		}
		output.buffer = NULL;
		output.curr = NULL;
		output.max = ULONG_MAX;
		if (use_gpu) {
			st = snappy_resize_gpu(&input, keep_len, tail_path ? &tail : NULL, &output, &rt);
		} else {
			gettimeofday(&t0, NULL);
			st = snappy_resize_host(&input, keep_len, tail_path ? &tail : NULL, &output);
			gettimeofday(&t1, NULL);
			rt.run = get_runtime(&t0, &t1);
		}
		if (tail_pinned)
			snappy_hip_host_free(tail.buffer);
		else
			free(tail.buffer);
	} else if (use_range) {
		/* only the blocks the range touches are decoded; the output holds exactly the range's bytes */
		output.buffer = NULL;
		output.curr = NULL;
		output.max = ULONG_MAX;
		if (use_gpu) {
			st = snappy_decompress_range_gpu(&input, &output, range_off, range_len, &rt);
		} else {
			gettimeofday(&t0, NULL);
			st = snappy_decompress_range_host(&input, &output, range_off, range_len);
			gettimeofday(&t1, NULL);
			rt.run = get_runtime(&t0, &t1);
		}
	} else if (use_gpu && use_wide) {
		/* a workgroup per block; the library reads the header itself and allocates the output (host mode ignores -W) */
		output.buffer = NULL;
		output.curr = NULL;
		output.max = ULONG_MAX;
		st = snappy_decompress_wide_gpu(&input, &output, (uint32_t)wide_waves, &rt);
	} else {
		if (setup_decompression(&input, &output, &rt))
			return -1;
		if (use_gpu && g_pinned) {           /* swap the malloc'd plaintext buffer for a page-locked one */
			free(output.buffer);
			output.buffer = buffer_alloc((output.length + 7) & ~7UL);
			output.curr = output.buffer;
		}
		if (use_gpu) {
			st = snappy_decompress_gpu(&input, &output, &rt);
		} else {
			gettimeofday(&t0, NULL);
			st = snappy_decompress_host(&input, &output);
			gettimeofday(&t1, NULL);
			rt.run = get_runtime(&t0, &t1);
		}
	}

	if (st != SNAPPY_OK) {
		fprintf(stderr, "Encountered Snappy error %u\n", st);   /* dpu_snappy.c:229-233 */
		return -1;
	}
	/* unlike snappy_compress_dpu (snappy_compress.c:626-627) the GPU path hands the stream back in
	 * output.buffer, so main writes the file in every mode */
	if (spill(out_path, &output))
		return -1;

	if (compress || use_write || use_resize) {          /* (-w, -t, -a: the new stream against the old one) */
		printf("Compressed %ld bytes to: %s\n", output.length, out_path);
		printf("Compression ratio: %f\n", 1 - (double)output.length / (double)input.length);
	} else {
		printf("Decompressed %ld bytes to: %s\n", output.length, out_path);
		printf("Compression ratio: %f\n", 1 - (double)input.length / (double)output.length);
	}
	printf("Pre-processing time: %f\n", rt.pre);
	printf("Alloc time: %f\n", rt.d_alloc);
	printf("Load time: %f\n", rt.load);
	printf("Copy in time: %f\n", rt.copy_in);
	printf("Host time: %f\n", rt.run);
	printf("Copy out time: %f\n", rt.copy_out);
	printf("Free time: %f\n", rt.d_free);
	return 0;
}
