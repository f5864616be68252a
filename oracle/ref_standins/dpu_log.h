/* No DPU log in this build; see dpu.h in this directory. */
