// What the two sources of the T2I-Adapter library share (include/minsdtf_hip_t2i.h).
#pragma once
#include <stdint.h>

// whether the byte ranges [a0, a1) and [b0, b1) meet
static inline bool msda_overlap(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }
