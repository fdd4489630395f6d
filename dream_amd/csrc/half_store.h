// The stored-value rule of activation_storage="fp16", in one place for every kernel that writes such a tensor (conv_f16_epilogue.inc,
// conv_first_body.inc, elementwise.hip): plain IEEE half, saturated to the largest finite half (never inf), rounded to nearest even,
// subnormals kept.
#pragma once
#include <dream_cdna4.h>

DREAM_DEVICE _Float16 sat_half(float v) { return (_Float16)fminf(fmaxf(v, -65504.0f), 65504.0f); }
