"""Which kernel every 3x3 convolution and mix of the model gets (mz_select.h: choose_conv3 / choose_mix), read without a GPU through
mz_debug_select().  That entry only maps its op code to a layer role; the role functions (conv1_call, conv2_call, d2s_call, ..) then
describe the call, a Conv3Call, exactly as they do for mz_forward and the mz_op_* entries, so a row here exercises the code the model
runs.  The expected names are those mz_debug_last_kernel() reported for these layers when the selection was spread over the
launch code; a row that changes is a change of the kernel that runs, and belongs in a pull request that says so."""

import pytest

from op_util import select_op, set_knobs
from ultrazoom_amd import _ffi

F32, BF16, F16 = _ffi.MZ_F32, _ffi.MZ_BF16, _ffi.MZ_F16
# mz_debug_select's ops (include/mewzoom_hip.h)
CONV1, CONV, UP, HEAD, QA, FILM, CONV2, MIX = range(8)
CUS = 256  # MI355X

# (dtype, op, cin, cout, B, H, W, knobs, kernel).  Every distinct 3x3 / mix layer of bench.py's workloads (UP: cout = 4 x the shuffled
# channels; CONV2: cin = the hidden channels, the fused family where mz_forward fuses conv2 and the mix; MIX: the unfused mix, cin = 2 cout).
# None: the launch is refused.
TABLE = [
    # cfg3_1080p, bf16, the default micro-batch of 3 images
    (BF16, CONV1, 96, 192, 3, 1080, 1920, '', 'conv3r'),
    (BF16, CONV2, 192, 96, 3, 1080, 1920, '', 'conv3r_fused'),
    (BF16, CONV1, 192, 384, 3, 540, 960, '', 'conv3r'),
    (BF16, CONV2, 384, 192, 3, 540, 960, '', 'conv3r'),
    (BF16, MIX, 384, 192, 3, 540, 960, '', 'mix16b'),
    (BF16, CONV1, 384, 768, 3, 270, 480, '', 'conv3r'),
    (BF16, CONV2, 768, 384, 3, 270, 480, '', 'conv3r'),
    (BF16, MIX, 768, 384, 3, 270, 480, '', 'mix16'),
    (BF16, CONV1, 768, 1536, 3, 135, 240, '', 'conv3r'),
    (BF16, CONV2, 1536, 768, 3, 135, 240, '', 'conv3r'),
    (BF16, MIX, 1536, 768, 3, 135, 240, '', 'mix16'),
    (BF16, QA, 768, 3, 3, 135, 240, '', 'conv3s'),
    (BF16, UP, 768, 1536, 3, 135, 240, '', 'conv3r'),
    (BF16, UP, 384, 768, 3, 270, 480, '', 'conv3r'),
    (BF16, UP, 192, 384, 3, 540, 960, '', 'conv3r'),
    (BF16, MIX, 192, 96, 3, 1080, 1920, '', 'conv_kernel_mix'),
    (BF16, UP, 96, 384, 3, 1080, 1920, '', 'conv3r'),
    (BF16, CONV1, 96, 192, 3, 2160, 3840, '', 'conv3r'),
    (BF16, CONV2, 192, 96, 3, 2160, 3840, '', 'conv3r_fused'),
    (BF16, HEAD, 96, 12, 3, 2160, 3840, '', 'conv_kernel'),
    # cfg3_540p, bf16, the default micro-batch of 15 images
    (BF16, CONV1, 96, 192, 15, 540, 960, '', 'conv3r'),
    (BF16, CONV2, 192, 96, 15, 540, 960, '', 'conv3r_fused'),
    (BF16, CONV1, 192, 384, 15, 270, 480, '', 'conv3r'),
    (BF16, CONV2, 384, 192, 15, 270, 480, '', 'conv3r'),
    (BF16, MIX, 384, 192, 15, 270, 480, '', 'mix16b'),
    (BF16, CONV1, 384, 768, 15, 135, 240, '', 'conv3r'),
    (BF16, CONV2, 768, 384, 15, 135, 240, '', 'conv3r'),
    (BF16, MIX, 768, 384, 15, 135, 240, '', 'mix16'),
    (BF16, CONV1, 768, 1536, 15, 67, 120, '', 'conv3r_8x40'),
    (BF16, CONV2, 1536, 768, 15, 67, 120, '', 'conv3r_8x40'),
    (BF16, MIX, 1536, 768, 15, 67, 120, '', 'mix16'),
    (BF16, QA, 768, 3, 15, 67, 120, '', 'conv3s'),
    (BF16, UP, 768, 1536, 15, 67, 120, '', 'conv3r_8x40'),
    (BF16, UP, 384, 768, 15, 135, 240, '', 'conv3r'),
    (BF16, UP, 192, 384, 15, 270, 480, '', 'conv3r'),
    (BF16, MIX, 192, 96, 15, 540, 960, '', 'conv_kernel_mix'),
    (BF16, UP, 96, 384, 15, 540, 960, '', 'conv3r'),
    (BF16, CONV1, 96, 192, 15, 1080, 1920, '', 'conv3r'),
    (BF16, CONV2, 192, 96, 15, 1080, 1920, '', 'conv3r_fused'),
    (BF16, HEAD, 96, 12, 15, 1080, 1920, '', 'conv_kernel'),
    # cfg2, bf16, 32 images
    (BF16, CONV1, 48, 96, 32, 540, 960, '', 'conv3r_ragged'),
    (BF16, CONV2, 96, 48, 32, 540, 960, '', 'conv3t_fused'),
    (BF16, CONV1, 96, 192, 32, 270, 480, '', 'conv3r'),
    (BF16, CONV2, 192, 96, 32, 270, 480, '', 'conv3r_fused'),
    (BF16, CONV1, 192, 384, 32, 135, 240, '', 'conv3r'),
    (BF16, CONV2, 384, 192, 32, 135, 240, '', 'conv3r'),
    (BF16, MIX, 384, 192, 32, 135, 240, '', 'mix16b'),
    (BF16, CONV1, 384, 768, 32, 67, 120, '', 'conv3r_8x40'),
    (BF16, CONV2, 768, 384, 32, 67, 120, '', 'conv3r_8x40'),
    (BF16, MIX, 768, 384, 32, 67, 120, '', 'mix16'),
    (BF16, QA, 384, 3, 32, 67, 120, '', 'conv3s'),
    (BF16, UP, 384, 768, 32, 67, 120, '', 'conv3r_8x40'),
    (BF16, UP, 192, 384, 32, 135, 240, '', 'conv3r'),
    (BF16, MIX, 192, 96, 32, 270, 480, '', 'conv_kernel_mix'),
    (BF16, UP, 96, 192, 32, 270, 480, '', 'conv3r'),
    (BF16, MIX, 96, 48, 32, 540, 960, '', 'conv_kernel_mix'),
    (BF16, HEAD, 48, 12, 32, 540, 960, '', 'conv_kernel'),
    # cfg3_1080p, f16
    (F16, CONV1, 96, 192, 3, 1080, 1920, '', 'conv3r'),
    (F16, CONV2, 192, 96, 3, 1080, 1920, '', 'conv3r_fused'),
    (F16, CONV1, 192, 384, 3, 540, 960, '', 'conv3r'),
    (F16, CONV2, 384, 192, 3, 540, 960, '', 'conv3r'),
    (F16, MIX, 384, 192, 3, 540, 960, '', 'mix16b'),
    (F16, CONV1, 384, 768, 3, 270, 480, '', 'conv3r'),
    (F16, CONV2, 768, 384, 3, 270, 480, '', 'conv3r'),
    (F16, MIX, 768, 384, 3, 270, 480, '', 'mix16'),
    (F16, CONV1, 768, 1536, 3, 135, 240, '', 'conv3r'),
    (F16, CONV2, 1536, 768, 3, 135, 240, '', 'conv3r'),
    (F16, MIX, 1536, 768, 3, 135, 240, '', 'mix16'),
    (F16, QA, 768, 3, 3, 135, 240, '', 'conv3s'),
    (F16, UP, 768, 1536, 3, 135, 240, '', 'conv3r'),
    (F16, UP, 384, 768, 3, 270, 480, '', 'conv3r'),
    (F16, UP, 192, 384, 3, 540, 960, '', 'conv3r'),
    (F16, MIX, 192, 96, 3, 1080, 1920, '', 'conv_kernel_mix'),
    (F16, UP, 96, 384, 3, 1080, 1920, '', 'conv3r'),
    (F16, CONV1, 96, 192, 3, 2160, 3840, '', 'conv3r'),
    (F16, CONV2, 192, 96, 3, 2160, 3840, '', 'conv3r_fused'),
    (F16, HEAD, 96, 12, 3, 2160, 3840, '', 'conv_kernel'),
    # cfg3_1080p, f32
    (F32, CONV1, 96, 192, 3, 1080, 1920, '', 'conv3p'),
    (F32, CONV2, 192, 96, 3, 1080, 1920, '', 'conv3w_fused'),
    (F32, CONV1, 192, 384, 3, 540, 960, '', 'conv3p'),
    (F32, CONV2, 384, 192, 3, 540, 960, '', 'conv3p'),
    (F32, MIX, 384, 192, 3, 540, 960, '', 'conv_kernel_mix'),
    (F32, CONV1, 384, 768, 3, 270, 480, '', 'conv3p'),
    (F32, CONV2, 768, 384, 3, 270, 480, '', 'conv3p'),
    (F32, MIX, 768, 384, 3, 270, 480, '', 'conv_kernel_mix'),
    (F32, CONV1, 768, 1536, 3, 135, 240, '', 'conv3p'),
    (F32, CONV2, 1536, 768, 3, 135, 240, '', 'conv3p'),
    (F32, MIX, 1536, 768, 3, 135, 240, '', 'conv_kernel_mix'),
    (F32, QA, 768, 3, 3, 135, 240, '', 'conv3w'),
    (F32, UP, 768, 1536, 3, 135, 240, '', 'conv3p'),
    (F32, UP, 384, 768, 3, 270, 480, '', 'conv3p'),
    (F32, UP, 192, 384, 3, 540, 960, '', 'conv3p'),
    (F32, MIX, 192, 96, 3, 1080, 1920, '', 'conv_kernel_mix'),
    (F32, UP, 96, 384, 3, 1080, 1920, '', 'conv3p'),
    (F32, CONV1, 96, 192, 3, 2160, 3840, '', 'conv3p'),
    (F32, CONV2, 192, 96, 3, 2160, 3840, '', 'conv3w_fused'),
    (F32, HEAD, 96, 12, 3, 2160, 3840, '', 'conv3w'),
    # cfg2, f32
    (F32, CONV1, 48, 96, 32, 540, 960, '', 'conv3p'),
    (F32, CONV2, 96, 48, 32, 540, 960, '', 'conv3w_fused'),
    (F32, CONV1, 96, 192, 32, 270, 480, '', 'conv3p'),
    (F32, CONV2, 192, 96, 32, 270, 480, '', 'conv3w_fused'),
    (F32, CONV1, 192, 384, 32, 135, 240, '', 'conv3p'),
    (F32, CONV2, 384, 192, 32, 135, 240, '', 'conv3p'),
    (F32, MIX, 384, 192, 32, 135, 240, '', 'conv_kernel_mix'),
    (F32, CONV1, 384, 768, 32, 67, 120, '', 'conv3p'),
    (F32, CONV2, 768, 384, 32, 67, 120, '', 'conv3p'),
    (F32, MIX, 768, 384, 32, 67, 120, '', 'conv_kernel_mix'),
    (F32, QA, 384, 3, 32, 67, 120, '', 'conv3p'),
    (F32, UP, 384, 768, 32, 67, 120, '', 'conv3p'),
    (F32, UP, 192, 384, 32, 135, 240, '', 'conv3p'),
    (F32, MIX, 192, 96, 32, 270, 480, '', 'conv_kernel_mix'),
    (F32, UP, 96, 192, 32, 270, 480, '', 'conv3p'),
    (F32, MIX, 96, 48, 32, 540, 960, '', 'conv_kernel_mix'),
    (F32, HEAD, 48, 12, 32, 540, 960, '', 'conv3w'),
    # fixture models, C = 16, 37 x 45 (bf16)
    (BF16, CONV1, 16, 32, 1, 37, 45, '', 'conv3w'),
    (BF16, CONV2, 32, 16, 1, 37, 45, '', 'conv3s_fused'),
    (BF16, CONV1, 32, 64, 1, 18, 22, '', 'conv3s'),
    (BF16, CONV2, 64, 32, 1, 18, 22, '', 'conv3s_fused'),
    (BF16, CONV1, 64, 128, 1, 9, 11, '', 'conv3s'),
    (BF16, CONV2, 128, 64, 1, 9, 11, '', 'conv3s_fused'),
    (BF16, CONV1, 128, 256, 1, 4, 5, '', 'conv3s'),
    (BF16, CONV2, 256, 128, 1, 4, 5, '', 'conv3s'),
    (BF16, MIX, 256, 128, 1, 4, 5, '', 'conv_kernel_mix'),
    (BF16, QA, 128, 3, 1, 4, 5, '', 'conv3s'),
    (BF16, UP, 128, 256, 1, 4, 5, '', 'conv3s'),
    (BF16, MIX, 128, 64, 1, 9, 11, '', 'conv_kernel_mix'),
    (BF16, UP, 64, 128, 1, 9, 11, '', 'conv3s'),
    (BF16, MIX, 64, 32, 1, 18, 22, '', 'conv_kernel_mix'),
    (BF16, UP, 32, 64, 1, 18, 22, '', 'conv3s'),
    (BF16, MIX, 32, 16, 1, 37, 45, '', 'conv_kernel_mix'),
    (BF16, UP, 16, 64, 1, 37, 45, '', 'conv3w'),
    (BF16, CONV1, 16, 32, 1, 74, 90, '', 'conv3w'),
    (BF16, CONV2, 32, 16, 1, 74, 90, '', 'conv3s_fused'),
    (BF16, HEAD, 16, 12, 1, 74, 90, '', 'conv_kernel'),
    # fixture models, C = 16, 64 x 120 (f16)
    (F16, CONV1, 16, 32, 2, 64, 120, '', 'conv3w'),
    (F16, CONV2, 32, 16, 2, 64, 120, '', 'conv3s_fused'),
    (F16, CONV1, 32, 64, 2, 32, 60, '', 'conv3s'),
    (F16, CONV2, 64, 32, 2, 32, 60, '', 'conv3s_fused'),
    (F16, CONV1, 64, 128, 2, 16, 30, '', 'conv3s'),
    (F16, CONV2, 128, 64, 2, 16, 30, '', 'conv3s_fused'),
    (F16, CONV1, 128, 256, 2, 8, 15, '', 'conv3s'),
    (F16, CONV2, 256, 128, 2, 8, 15, '', 'conv3s'),
    (F16, MIX, 256, 128, 2, 8, 15, '', 'conv_kernel_mix'),
    (F16, QA, 128, 3, 2, 8, 15, '', 'conv3s'),
    (F16, UP, 128, 256, 2, 8, 15, '', 'conv3s'),
    (F16, MIX, 128, 64, 2, 16, 30, '', 'conv_kernel_mix'),
    (F16, UP, 64, 128, 2, 16, 30, '', 'conv3s'),
    (F16, MIX, 64, 32, 2, 32, 60, '', 'conv_kernel_mix'),
    (F16, UP, 32, 64, 2, 32, 60, '', 'conv3s'),
    (F16, MIX, 32, 16, 2, 64, 120, '', 'conv_kernel_mix'),
    (F16, HEAD, 16, 12, 2, 64, 120, '', 'conv_kernel'),
    # fixture models, C = 24, 37 x 45 (bf16)
    (BF16, CONV1, 24, 48, 1, 37, 45, '', 'conv3s'),
    (BF16, CONV2, 48, 24, 1, 37, 45, '', 'conv3w_fused'),
    (BF16, CONV1, 40, 80, 1, 18, 22, '', 'conv3r_ragged'),
    (BF16, CONV2, 80, 40, 1, 18, 22, '', 'conv3w_fused'),
    (BF16, CONV1, 72, 144, 1, 9, 11, '', 'conv3w'),
    (BF16, CONV2, 144, 72, 1, 9, 11, '', 'conv3s_fused'),
    (BF16, CONV1, 136, 272, 1, 4, 5, '', 'conv3s'),
    (BF16, CONV2, 272, 136, 1, 4, 5, '', 'conv3s'),
    (BF16, MIX, 272, 136, 1, 4, 5, '', 'conv_kernel_mix'),
    (BF16, QA, 136, 3, 1, 4, 5, '', 'conv3s'),
    (BF16, UP, 136, 288, 1, 4, 5, '', 'conv3s'),
    (BF16, MIX, 144, 72, 1, 9, 11, '', 'conv_kernel_mix'),
    (BF16, UP, 72, 160, 1, 9, 11, '', 'conv3w'),
    (BF16, MIX, 80, 40, 1, 18, 22, '', 'conv_kernel_mix'),
    (BF16, UP, 40, 96, 1, 18, 22, '', 'conv3w'),
    (BF16, MIX, 48, 24, 1, 37, 45, '', 'conv_kernel_mix'),
    (BF16, UP, 24, 96, 1, 37, 45, '', 'conv3s'),
    (BF16, CONV1, 24, 48, 1, 74, 90, '', 'conv3s'),
    (BF16, CONV2, 48, 24, 1, 74, 90, '', 'conv3w_fused'),
    (BF16, HEAD, 24, 12, 1, 74, 90, '', 'conv_kernel'),
    # fixture models, C = 24, 64 x 120 (f16)
    (F16, CONV1, 24, 48, 2, 64, 120, '', 'conv3s'),
    (F16, CONV2, 48, 24, 2, 64, 120, '', 'conv3w_fused'),
    (F16, CONV1, 40, 80, 2, 32, 60, '', 'conv3r_ragged'),
    (F16, CONV2, 80, 40, 2, 32, 60, '', 'conv3w_fused'),
    (F16, CONV1, 72, 144, 2, 16, 30, '', 'conv3w'),
    (F16, CONV2, 144, 72, 2, 16, 30, '', 'conv3s_fused'),
    (F16, CONV1, 136, 272, 2, 8, 15, '', 'conv3s'),
    (F16, CONV2, 272, 136, 2, 8, 15, '', 'conv3s'),
    (F16, MIX, 272, 136, 2, 8, 15, '', 'conv_kernel_mix'),
    (F16, QA, 136, 3, 2, 8, 15, '', 'conv3s'),
    (F16, UP, 136, 288, 2, 8, 15, '', 'conv3s'),
    (F16, MIX, 144, 72, 2, 16, 30, '', 'conv_kernel_mix'),
    (F16, UP, 72, 160, 2, 16, 30, '', 'conv3w'),
    (F16, MIX, 80, 40, 2, 32, 60, '', 'conv_kernel_mix'),
    (F16, UP, 40, 96, 2, 32, 60, '', 'conv3w'),
    (F16, MIX, 48, 24, 2, 64, 120, '', 'conv_kernel_mix'),
    (F16, HEAD, 24, 12, 2, 64, 120, '', 'conv_kernel'),
    # fixture models, C = 32, 37 x 45 (bf16)
    (BF16, CONV1, 32, 64, 1, 37, 45, '', 'conv3s'),
    (BF16, CONV2, 64, 32, 1, 37, 45, '', 'conv3s_fused'),
    (BF16, CONV1, 64, 128, 1, 18, 22, '', 'conv3s'),
    (BF16, CONV2, 128, 64, 1, 18, 22, '', 'conv3s_fused'),
    (BF16, CONV1, 128, 256, 1, 9, 11, '', 'conv3s'),
    (BF16, CONV2, 256, 128, 1, 9, 11, '', 'conv3s'),
    (BF16, MIX, 256, 128, 1, 9, 11, '', 'conv_kernel_mix'),
    (BF16, CONV1, 256, 512, 1, 4, 5, '', 'conv3s'),
    (BF16, CONV2, 512, 256, 1, 4, 5, '', 'conv3s'),
    (BF16, MIX, 512, 256, 1, 4, 5, '', 'conv_kernel_mix'),
    (BF16, QA, 256, 3, 1, 4, 5, '', 'conv3s'),
    (BF16, UP, 256, 512, 1, 4, 5, '', 'conv3s'),
    (BF16, UP, 128, 256, 1, 9, 11, '', 'conv3s'),
    (BF16, MIX, 128, 64, 1, 18, 22, '', 'conv_kernel_mix'),
    (BF16, UP, 64, 128, 1, 18, 22, '', 'conv3s'),
    (BF16, MIX, 64, 32, 1, 37, 45, '', 'conv_kernel_mix'),
    (BF16, UP, 32, 128, 1, 37, 45, '', 'conv3s'),
    (BF16, CONV1, 32, 64, 1, 74, 90, '', 'conv3s'),
    (BF16, CONV2, 64, 32, 1, 74, 90, '', 'conv3s_fused'),
    (BF16, HEAD, 32, 12, 1, 74, 90, '', 'conv_kernel'),
    # fixture models, C = 32, 64 x 120 (f16)
    (F16, CONV1, 32, 64, 2, 64, 120, '', 'conv3s'),
    (F16, CONV2, 64, 32, 2, 64, 120, '', 'conv3s_fused'),
    (F16, CONV1, 64, 128, 2, 32, 60, '', 'conv3s'),
    (F16, CONV2, 128, 64, 2, 32, 60, '', 'conv3s_fused'),
    (F16, CONV1, 128, 256, 2, 16, 30, '', 'conv3s'),
    (F16, CONV2, 256, 128, 2, 16, 30, '', 'conv3s'),
    (F16, MIX, 256, 128, 2, 16, 30, '', 'conv_kernel_mix'),
    (F16, CONV1, 256, 512, 2, 8, 15, '', 'conv3s'),
    (F16, CONV2, 512, 256, 2, 8, 15, '', 'conv3s'),
    (F16, MIX, 512, 256, 2, 8, 15, '', 'conv_kernel_mix'),
    (F16, QA, 256, 3, 2, 8, 15, '', 'conv3s'),
    (F16, UP, 256, 512, 2, 8, 15, '', 'conv3s'),
    (F16, UP, 128, 256, 2, 16, 30, '', 'conv3s'),
    (F16, MIX, 128, 64, 2, 32, 60, '', 'conv_kernel_mix'),
    (F16, UP, 64, 128, 2, 32, 60, '', 'conv3s'),
    (F16, MIX, 64, 32, 2, 64, 120, '', 'conv_kernel_mix'),
    (F16, HEAD, 32, 12, 2, 64, 120, '', 'conv_kernel'),
    # hidden ratio 1 / 4 of the C = 16 fixtures
    (BF16, CONV2, 16, 16, 1, 37, 45, '', 'conv3w_fused'),
    (BF16, CONV1, 16, 64, 1, 37, 45, '', 'conv3w'),
    (BF16, CONV2, 64, 16, 1, 37, 45, '', 'conv3s_fused'),
    # widths where 8 x 40 tiles pad fewer pixels
    (BF16, CONV1, 96, 192, 1, 24, 120, '', 'conv3r_8x40'),
    (BF16, CONV, 96, 96, 2, 64, 120, '', 'conv3r_8x40'),
    (F16, UP, 192, 384, 1, 33, 120, '', 'conv3r_8x40'),
    (BF16, CONV, 96, 96, 1, 50, 190, '', 'conv3r'),
    # MZ_NO_R=1
    (BF16, CONV1, 96, 192, 3, 1080, 1920, 'MZ_NO_R=1', 'conv3s'),
    (BF16, CONV2, 192, 96, 3, 1080, 1920, 'MZ_NO_R=1', 'conv3s_fused'),
    (BF16, CONV1, 48, 96, 32, 270, 480, 'MZ_NO_R=1', 'conv3p'),
    (BF16, UP, 192, 384, 3, 540, 960, 'MZ_NO_R=1', 'conv3s'),
    # MZ_NO_T=1
    (BF16, CONV2, 96, 48, 32, 540, 960, 'MZ_NO_T=1', 'conv3s_fused'),
    (BF16, CONV1, 96, 48, 2, 36, 130, 'MZ_NO_T=1', 'conv3s'),
    # MZ_NO_R2=1
    (BF16, CONV1, 48, 96, 32, 540, 960, 'MZ_NO_R2=1', 'conv3p'),
    # MZ_NO_FUSE16=1
    (BF16, CONV2, 192, 96, 3, 1080, 1920, 'MZ_NO_FUSE16=1', 'conv3w_fused'),
    (BF16, CONV2, 96, 48, 32, 540, 960, 'MZ_NO_FUSE16=1', 'conv3w_fused'),
    (BF16, CONV2, 32, 16, 1, 37, 45, 'MZ_NO_FUSE16=1', 'conv3w_fused'),
    # MZ_NO_S16=1
    (BF16, CONV1, 96, 192, 3, 1080, 1920, 'MZ_NO_S16=1', 'conv3p'),
    (BF16, CONV2, 192, 96, 3, 1080, 1920, 'MZ_NO_S16=1', 'conv3p'),
    (BF16, CONV2, 96, 48, 32, 540, 960, 'MZ_NO_S16=1', 'conv3p'),
    (BF16, FILM, 96, 96, 1, 37, 45, 'MZ_NO_S16=1', None),
    # MZ_NO_WIDE=1
    (BF16, CONV1, 96, 192, 3, 1080, 1920, 'MZ_NO_WIDE=1', 'conv3r'),
    (BF16, CONV2, 192, 96, 3, 1080, 1920, 'MZ_NO_WIDE=1', 'conv3r'),
    (BF16, HEAD, 96, 12, 3, 2160, 3840, 'MZ_NO_WIDE=1', 'conv_kernel'),
    (F32, HEAD, 96, 12, 3, 2160, 3840, 'MZ_NO_WIDE=1', 'conv_kernel'),
    # MZ_NO_FUSE=1
    (BF16, CONV2, 192, 96, 3, 1080, 1920, 'MZ_NO_FUSE=1', 'conv3r'),
    (BF16, CONV2, 96, 48, 32, 540, 960, 'MZ_NO_FUSE=1', 'conv3t'),
    # MZ_NO_MIX16B=1
    (BF16, MIX, 384, 192, 3, 540, 960, 'MZ_NO_MIX16B=1', 'mix16'),
    (BF16, MIX, 768, 384, 3, 270, 480, 'MZ_NO_MIX16B=1', 'mix16'),
    # MZ_KPAD_PCT=0
    (BF16, CONV2, 48, 24, 1, 37, 45, 'MZ_KPAD_PCT=0', 'conv3w_fused'),
    (BF16, CONV1, 96, 192, 3, 1080, 1920, 'MZ_KPAD_PCT=0', 'conv3r'),
    # MZ_KPAD_PCT=50
    (BF16, CONV2, 48, 24, 1, 37, 45, 'MZ_KPAD_PCT=50', 'conv3s_fused'),
    (BF16, CONV1, 16, 32, 1, 37, 45, 'MZ_KPAD_PCT=50', 'conv3w'),
    # MZ_PERSIST_WGS=8
    (BF16, CONV1, 96, 192, 1, 37, 45, 'MZ_PERSIST_WGS=8', 'conv3r'),
    (BF16, CONV, 16, 16, 1, 37, 45, 'MZ_PERSIST_WGS=8', 'conv3w'),
    (BF16, MIX, 384, 192, 1, 37, 45, 'MZ_PERSIST_WGS=8', 'mix16b'),
    # MZ_NO_PERSIST=1
    (BF16, CONV1, 96, 192, 3, 1080, 1920, 'MZ_NO_PERSIST=1', 'conv3w'),
    (BF16, CONV2, 192, 96, 3, 1080, 1920, 'MZ_NO_PERSIST=1', 'conv3w_fused'),
    (BF16, CONV2, 96, 48, 32, 540, 960, 'MZ_NO_PERSIST=1', 'conv3w_fused'),
    (BF16, MIX, 384, 192, 3, 540, 960, 'MZ_NO_PERSIST=1', 'mix16b'),
    (BF16, MIX, 768, 384, 3, 270, 480, 'MZ_NO_PERSIST=1', 'mix16'),
    # FiLM: on conv3s, refused where Cin pads badly to 32-channel chunks, refused in f32
    (BF16, FILM, 96, 96, 2, 37, 45, '', 'conv3s'),
    (F16, FILM, 32, 64, 2, 37, 45, '', 'conv3s'),
    (BF16, FILM, 48, 96, 2, 37, 45, '', None),
    (F32, FILM, 96, 96, 2, 37, 45, '', None),
]


def _select(monkeypatch, dtype, op, cin, cout, B, H, W, env=""):
    set_knobs(monkeypatch, dict(kv.split("=") for kv in env.split()))  # each row sees only its own knobs
    return select_op(dtype, op, cin, cout, B, H, W, CUS), _ffi.lib().mz_last_error().decode()


@pytest.mark.parametrize("row", TABLE, ids=lambda r: "-".join(str(v) for v in r[:7]) + ("-" + r[7].replace(" ", "+") if r[7] else ""))
def test_kernel_selection_table(row, monkeypatch):
    *args, env, want = row
    got, _ = _select(monkeypatch, *args, env)
    assert got == want


def test_refusals_say_why(monkeypatch):
    got, err = _select(monkeypatch, BF16, FILM, 48, 96, 2, 37, 45)
    assert got is None and "16x16x32" in err
    got, err = _select(monkeypatch, F32, FILM, 96, 96, 2, 37, 45)
    assert got is None and "bf16 / fp16" in err
    got, err = _select(monkeypatch, BF16, 8, 96, 96, 1, 37, 45)
    assert got is None and "bad op" in err
    # conv3r's tile list holds pixel coordinates in 16 bits
    got, err = _select(monkeypatch, BF16, CONV1, 96, 192, 1, 16, 70000)
    assert got is None and "16 bits" in err


def test_planning_and_selection_survive_the_sanitizers(tmp_path):
    """tests/select_main.cpp -- planned models and their schedules (liveness and extents of every operand), then the layers of those
    schedules and channel counts around every tile and chunk boundary, 8 x 8 to 4320 x 7680 pixels, 1 to 64 images, 0 / 8 / 256 CUs:
    plans, choices, walks, tile lists (every tile exactly once) and workspace plans -- built from mz_plan.h, mz_select.h and
    mz_schedule.h alone with the address and undefined-behaviour sanitizers: a signed overflow in a tile count or an offset
    guard ends it.  A stand-alone host program: nothing of it is loaded here, nothing of HIP is linked."""
    import os
    import shutil
    import subprocess
    from pathlib import Path

    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    rocm_include = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")  # hipError_t / hipStream_t of mz_kernels.h: types only
    src = Path(__file__).resolve().parent / "select_main.cpp"
    exe = tmp_path / "select_main"
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + rocm_include,
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", str(src), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "selection OK" in run.stdout and not run.stderr, (run.returncode, run.stdout[-2000:], run.stderr[-3000:])
