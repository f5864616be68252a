/* No DPU memory interface in this build; see dpu.h in this directory. */
