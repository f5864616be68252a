/* Stand-in for the PIM vendor's host header.  There is no DPU in this build: the reference codec's sources are compiled
 * for their host path alone (oracle/Makefile, target `ref`), and every DPU entry point they name ends the process with a
 * message and exit status 70 + k, so a test that takes the DPU path by mistake cannot pass for a codec result. */
#ifndef REF_STANDIN_DPU_H
#define REF_STANDIN_DPU_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

struct dpu_set_t {
    int none;
};

typedef enum { DPU_XFER_TO_DPU, DPU_XFER_FROM_DPU } dpu_xfer_t;
typedef enum { DPU_XFER_DEFAULT } dpu_xfer_flags_t;
typedef enum { DPU_SYNCHRONOUS, DPU_ASYNCHRONOUS } dpu_launch_policy_t;

static inline int ref_standin_no_dpu(const char *call, int k)
{
    fprintf(stderr, "%s: no DPU in this build (host path only)\n", call);
    exit(70 + k);
    return 0;
}

#define DPU_ASSERT(call) ((void)(call))
/* the loop bodies are never reached: the allocation in front of them has already ended the process */
#define DPU_FOREACH(set, one) for ((one) = (set); ref_standin_no_dpu("DPU_FOREACH", 10);)
#define DPU_RANK_FOREACH(set, one) for ((one) = (set); ref_standin_no_dpu("DPU_RANK_FOREACH", 11);)

#define dpu_alloc(...) ref_standin_no_dpu("dpu_alloc", 0)
#define dpu_load(...) ref_standin_no_dpu("dpu_load", 1)
#define dpu_prepare_xfer(...) ref_standin_no_dpu("dpu_prepare_xfer", 2)
#define dpu_push_xfer(...) ref_standin_no_dpu("dpu_push_xfer", 3)
#define dpu_copy_to(...) ref_standin_no_dpu("dpu_copy_to", 4)
#define dpu_copy_from(...) ref_standin_no_dpu("dpu_copy_from", 5)
#define dpu_launch(...) ref_standin_no_dpu("dpu_launch", 6)
#define dpu_free(...) ref_standin_no_dpu("dpu_free", 7)
#define dpu_get_nr_dpus(...) ref_standin_no_dpu("dpu_get_nr_dpus", 8)
#define dpu_log_read(...) ref_standin_no_dpu("dpu_log_read", 9)

#endif
