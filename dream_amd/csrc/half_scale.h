// The power-of-two scales of the fp16 training kernels, derived on the device from an amax scalar (the bit pattern of a non-negative
// float), in one place for wgrad_f16.hip and conv_f16.hip.
#pragma once
#include <dream_cdna4.h>

// e with max|t| * 2^e in [2^13, 2^14): 13 - exponent, clamped to +-100; 0 for a zero tensor (conv_f16.hip).  The per-tensor scale of an
// fp32 operand that is rounded to half while it is staged.
DREAM_DEVICE int scale_exponent(unsigned amax_bits) {
    const int e = (amax_bits == 0u) ? 0 : 13 - ((int)((amax_bits >> 23) & 255) - 127);
    return e < -100 ? -100 : (e > 100 ? 100 : e);
}

// Its twin for the half-stored data gradients of one backward pass (train_gradient_storage="fp16"): e_g with max|dL/dy| * 2^e_g in
// [2^9, 2^10), from the amax of the LOSS gradient; every gradient of the run is stored times 2^e_g.
DREAM_DEVICE int grad_scale_exponent(unsigned amax_bits) {
    const int e = (amax_bits == 0u) ? 0 : 9 - ((int)((amax_bits >> 23) & 255) - 127);
    return e < -100 ? -100 : (e > 100 ? 100 : e);
}
