"""The weight packings of every layer (PackLayout, ultrazoom_amd/csrc/mz_kernels.h), read without a GPU through mz_debug_pack(): which
packings a layer has, how many bytes each takes, and that each one holds every real weight exactly once (pack_kernel runs the same map,
mz_pack.h).  The table was recorded from the planned sizes of ConvW's packings when they were four pointer / size pairs (packed,
packed16, packed16r, packed16t); a row that changes is a change of what the kernels read, and belongs in a pull request that says so."""

import numpy as np
import pytest

from ultrazoom_amd import _ffi

F32, BF16, F16 = _ffi.MZ_F32, _ffi.MZ_BF16, _ffi.MZ_F16
# mz_debug_select's ops (include/mewzoom_hip.h); GATE = the gate weights of a block's mix packed for the fused conv2 + mix (cin, cout: conv2's)
CONV1, CONV, UP, HEAD, QA, FILM, CONV2, MIX, GATE = range(9)
# PackLayout, in order
LAYOUTS = ("main", "conv16", "mix16", "gate16", "mix16b", "gate16r", "conv16t", "gate16t")

# (dtype, op, cin, cout, {layout: planned bytes}): one row per distinct layer of tests/test_select_cpu.TABLE (and the fused gate of its
# conv2 rows where the block fuses), for every dtype
TABLE = [
    # bf16
    (BF16, CONV1, 96, 192, {'main': 331776, 'conv16': 331776}),
    (BF16, CONV2, 192, 96, {'main': 331776, 'conv16': 331776}),
    (BF16, GATE, 192, 96, {'main': 36864, 'gate16': 36864, 'gate16r': 36864}),
    (BF16, CONV1, 192, 384, {'main': 1327104, 'conv16': 1327104}),
    (BF16, CONV2, 384, 192, {'main': 1327104, 'conv16': 1327104}),
    (BF16, MIX, 384, 192, {'main': 147456, 'mix16': 147456, 'mix16b': 147456}),
    (BF16, CONV1, 384, 768, {'main': 5308416, 'conv16': 5308416}),
    (BF16, CONV2, 768, 384, {'main': 5308416, 'conv16': 5308416}),
    (BF16, MIX, 768, 384, {'main': 589824, 'mix16': 589824}),
    (BF16, CONV1, 768, 1536, {'main': 21233664, 'conv16': 21233664}),
    (BF16, CONV2, 1536, 768, {'main': 21233664, 'conv16': 21233664}),
    (BF16, MIX, 1536, 768, {'main': 2359296, 'mix16': 2359296}),
    (BF16, QA, 768, 3, {'main': 442368, 'conv16': 442368}),
    (BF16, UP, 768, 1536, {'main': 21233664, 'conv16': 21233664}),
    (BF16, UP, 384, 768, {'main': 5308416, 'conv16': 5308416}),
    (BF16, UP, 192, 384, {'main': 1327104, 'conv16': 1327104}),
    (BF16, MIX, 192, 96, {'main': 36864}),
    (BF16, UP, 96, 384, {'main': 663552, 'conv16': 663552}),
    (BF16, HEAD, 96, 12, {'main': 55296}),
    (BF16, CONV1, 48, 96, {'main': 82944, 'conv16': 110592}),
    (BF16, CONV2, 96, 48, {'main': 110592, 'conv16': 110592, 'conv16t': 82944}),
    (BF16, GATE, 96, 48, {'main': 14336, 'gate16': 16384, 'gate16t': 9216}),
    (BF16, QA, 384, 3, {'main': 221184, 'conv16': 221184}),
    (BF16, UP, 96, 192, {'main': 331776, 'conv16': 331776}),
    (BF16, MIX, 96, 48, {'main': 12288}),
    (BF16, HEAD, 48, 12, {'main': 27648}),
    (BF16, CONV1, 16, 32, {'main': 9216, 'conv16': 18432}),
    (BF16, CONV2, 32, 16, {'main': 18432, 'conv16': 18432}),
    (BF16, GATE, 32, 16, {'main': 3072, 'gate16': 4096}),
    (BF16, CONV1, 32, 64, {'main': 36864, 'conv16': 36864}),
    (BF16, CONV2, 64, 32, {'main': 36864, 'conv16': 36864}),
    (BF16, GATE, 64, 32, {'main': 4096, 'gate16': 4096}),
    (BF16, CONV1, 64, 128, {'main': 147456, 'conv16': 147456}),
    (BF16, CONV2, 128, 64, {'main': 147456, 'conv16': 147456}),
    (BF16, GATE, 128, 64, {'main': 16384, 'gate16': 16384}),
    (BF16, CONV1, 128, 256, {'main': 589824, 'conv16': 589824}),
    (BF16, CONV2, 256, 128, {'main': 589824, 'conv16': 589824}),
    (BF16, MIX, 256, 128, {'main': 65536}),
    (BF16, QA, 128, 3, {'main': 73728, 'conv16': 73728}),
    (BF16, UP, 128, 256, {'main': 589824, 'conv16': 589824}),
    (BF16, MIX, 128, 64, {'main': 16384}),
    (BF16, UP, 64, 128, {'main': 147456, 'conv16': 147456}),
    (BF16, MIX, 64, 32, {'main': 4096}),
    (BF16, UP, 32, 64, {'main': 36864, 'conv16': 36864}),
    (BF16, MIX, 32, 16, {'main': 2048}),
    (BF16, UP, 16, 64, {'main': 18432, 'conv16': 36864}),
    (BF16, HEAD, 16, 12, {'main': 9216}),
    (BF16, CONV1, 24, 48, {'main': 36864, 'conv16': 36864, 'conv16t': 27648}),
    (BF16, CONV2, 48, 24, {'main': 27648, 'conv16': 36864}),
    (BF16, GATE, 48, 24, {'main': 4096, 'gate16': 4096}),
    (BF16, CONV1, 40, 80, {'main': 82944, 'conv16': 110592}),
    (BF16, CONV2, 80, 40, {'main': 92160, 'conv16': 110592}),
    (BF16, GATE, 80, 40, {'main': 14336, 'gate16': 16384, 'gate16t': 9216}),
    (BF16, CONV1, 72, 144, {'main': 230400, 'conv16': 276480}),
    (BF16, CONV2, 144, 72, {'main': 248832, 'conv16': 276480}),
    (BF16, GATE, 144, 72, {'main': 33792, 'gate16': 36864, 'gate16r': 36864}),
    (BF16, CONV1, 136, 272, {'main': 746496, 'conv16': 829440}),
    (BF16, CONV2, 272, 136, {'main': 783360, 'conv16': 829440}),
    (BF16, MIX, 272, 136, {'main': 92160}),
    (BF16, QA, 136, 3, {'main': 82944, 'conv16': 92160}),
    (BF16, UP, 136, 288, {'main': 829440, 'conv16': 921600}),
    (BF16, MIX, 144, 72, {'main': 30720}),
    (BF16, UP, 72, 160, {'main': 276480, 'conv16': 331776}),
    (BF16, MIX, 80, 40, {'main': 12288}),
    (BF16, UP, 40, 96, {'main': 110592, 'conv16': 147456}),
    (BF16, MIX, 48, 24, {'main': 4096}),
    (BF16, UP, 24, 96, {'main': 73728, 'conv16': 73728}),
    (BF16, HEAD, 24, 12, {'main': 18432}),
    (BF16, CONV1, 256, 512, {'main': 2359296, 'conv16': 2359296}),
    (BF16, CONV2, 512, 256, {'main': 2359296, 'conv16': 2359296}),
    (BF16, MIX, 512, 256, {'main': 262144}),
    (BF16, QA, 256, 3, {'main': 147456, 'conv16': 147456}),
    (BF16, UP, 256, 512, {'main': 2359296, 'conv16': 2359296}),
    (BF16, UP, 32, 128, {'main': 73728, 'conv16': 73728}),
    (BF16, HEAD, 32, 12, {'main': 18432}),
    (BF16, CONV2, 16, 16, {'main': 9216, 'conv16': 18432}),
    (BF16, GATE, 16, 16, {'main': 3072, 'gate16': 4096}),
    (BF16, CONV1, 16, 64, {'main': 18432, 'conv16': 36864}),
    (BF16, CONV2, 64, 16, {'main': 36864, 'conv16': 36864}),
    (BF16, GATE, 64, 16, {'main': 3072, 'gate16': 4096}),
    (BF16, CONV, 96, 96, {'main': 165888, 'conv16': 165888}),
    (BF16, CONV1, 96, 48, {'main': 110592, 'conv16': 110592, 'conv16t': 82944}),
    (BF16, FILM, 96, 96, {'main': 165888, 'conv16': 165888}),
    (BF16, CONV, 16, 16, {'main': 9216, 'conv16': 18432}),
    (BF16, FILM, 32, 64, {'main': 36864, 'conv16': 36864}),
    (BF16, FILM, 48, 96, {'main': 82944, 'conv16': 110592}),
    # f16
    (F16, CONV1, 96, 192, {'main': 331776, 'conv16': 331776}),
    (F16, CONV2, 192, 96, {'main': 331776, 'conv16': 331776}),
    (F16, GATE, 192, 96, {'main': 36864, 'gate16': 36864, 'gate16r': 36864}),
    (F16, CONV1, 192, 384, {'main': 1327104, 'conv16': 1327104}),
    (F16, CONV2, 384, 192, {'main': 1327104, 'conv16': 1327104}),
    (F16, MIX, 384, 192, {'main': 147456, 'mix16': 147456, 'mix16b': 147456}),
    (F16, CONV1, 384, 768, {'main': 5308416, 'conv16': 5308416}),
    (F16, CONV2, 768, 384, {'main': 5308416, 'conv16': 5308416}),
    (F16, MIX, 768, 384, {'main': 589824, 'mix16': 589824}),
    (F16, CONV1, 768, 1536, {'main': 21233664, 'conv16': 21233664}),
    (F16, CONV2, 1536, 768, {'main': 21233664, 'conv16': 21233664}),
    (F16, MIX, 1536, 768, {'main': 2359296, 'mix16': 2359296}),
    (F16, QA, 768, 3, {'main': 442368, 'conv16': 442368}),
    (F16, UP, 768, 1536, {'main': 21233664, 'conv16': 21233664}),
    (F16, UP, 384, 768, {'main': 5308416, 'conv16': 5308416}),
    (F16, UP, 192, 384, {'main': 1327104, 'conv16': 1327104}),
    (F16, MIX, 192, 96, {'main': 36864}),
    (F16, UP, 96, 384, {'main': 663552, 'conv16': 663552}),
    (F16, HEAD, 96, 12, {'main': 55296}),
    (F16, CONV1, 48, 96, {'main': 82944, 'conv16': 110592}),
    (F16, CONV2, 96, 48, {'main': 110592, 'conv16': 110592, 'conv16t': 82944}),
    (F16, GATE, 96, 48, {'main': 14336, 'gate16': 16384, 'gate16t': 9216}),
    (F16, QA, 384, 3, {'main': 221184, 'conv16': 221184}),
    (F16, UP, 96, 192, {'main': 331776, 'conv16': 331776}),
    (F16, MIX, 96, 48, {'main': 12288}),
    (F16, HEAD, 48, 12, {'main': 27648}),
    (F16, CONV1, 16, 32, {'main': 9216, 'conv16': 18432}),
    (F16, CONV2, 32, 16, {'main': 18432, 'conv16': 18432}),
    (F16, GATE, 32, 16, {'main': 3072, 'gate16': 4096}),
    (F16, CONV1, 32, 64, {'main': 36864, 'conv16': 36864}),
    (F16, CONV2, 64, 32, {'main': 36864, 'conv16': 36864}),
    (F16, GATE, 64, 32, {'main': 4096, 'gate16': 4096}),
    (F16, CONV1, 64, 128, {'main': 147456, 'conv16': 147456}),
    (F16, CONV2, 128, 64, {'main': 147456, 'conv16': 147456}),
    (F16, GATE, 128, 64, {'main': 16384, 'gate16': 16384}),
    (F16, CONV1, 128, 256, {'main': 589824, 'conv16': 589824}),
    (F16, CONV2, 256, 128, {'main': 589824, 'conv16': 589824}),
    (F16, MIX, 256, 128, {'main': 65536}),
    (F16, QA, 128, 3, {'main': 73728, 'conv16': 73728}),
    (F16, UP, 128, 256, {'main': 589824, 'conv16': 589824}),
    (F16, MIX, 128, 64, {'main': 16384}),
    (F16, UP, 64, 128, {'main': 147456, 'conv16': 147456}),
    (F16, MIX, 64, 32, {'main': 4096}),
    (F16, UP, 32, 64, {'main': 36864, 'conv16': 36864}),
    (F16, MIX, 32, 16, {'main': 2048}),
    (F16, UP, 16, 64, {'main': 18432, 'conv16': 36864}),
    (F16, HEAD, 16, 12, {'main': 9216}),
    (F16, CONV1, 24, 48, {'main': 36864, 'conv16': 36864, 'conv16t': 27648}),
    (F16, CONV2, 48, 24, {'main': 27648, 'conv16': 36864}),
    (F16, GATE, 48, 24, {'main': 4096, 'gate16': 4096}),
    (F16, CONV1, 40, 80, {'main': 82944, 'conv16': 110592}),
    (F16, CONV2, 80, 40, {'main': 92160, 'conv16': 110592}),
    (F16, GATE, 80, 40, {'main': 14336, 'gate16': 16384, 'gate16t': 9216}),
    (F16, CONV1, 72, 144, {'main': 230400, 'conv16': 276480}),
    (F16, CONV2, 144, 72, {'main': 248832, 'conv16': 276480}),
    (F16, GATE, 144, 72, {'main': 33792, 'gate16': 36864, 'gate16r': 36864}),
    (F16, CONV1, 136, 272, {'main': 746496, 'conv16': 829440}),
    (F16, CONV2, 272, 136, {'main': 783360, 'conv16': 829440}),
    (F16, MIX, 272, 136, {'main': 92160}),
    (F16, QA, 136, 3, {'main': 82944, 'conv16': 92160}),
    (F16, UP, 136, 288, {'main': 829440, 'conv16': 921600}),
    (F16, MIX, 144, 72, {'main': 30720}),
    (F16, UP, 72, 160, {'main': 276480, 'conv16': 331776}),
    (F16, MIX, 80, 40, {'main': 12288}),
    (F16, UP, 40, 96, {'main': 110592, 'conv16': 147456}),
    (F16, MIX, 48, 24, {'main': 4096}),
    (F16, UP, 24, 96, {'main': 73728, 'conv16': 73728}),
    (F16, HEAD, 24, 12, {'main': 18432}),
    (F16, CONV1, 256, 512, {'main': 2359296, 'conv16': 2359296}),
    (F16, CONV2, 512, 256, {'main': 2359296, 'conv16': 2359296}),
    (F16, MIX, 512, 256, {'main': 262144}),
    (F16, QA, 256, 3, {'main': 147456, 'conv16': 147456}),
    (F16, UP, 256, 512, {'main': 2359296, 'conv16': 2359296}),
    (F16, UP, 32, 128, {'main': 73728, 'conv16': 73728}),
    (F16, HEAD, 32, 12, {'main': 18432}),
    (F16, CONV2, 16, 16, {'main': 9216, 'conv16': 18432}),
    (F16, GATE, 16, 16, {'main': 3072, 'gate16': 4096}),
    (F16, CONV1, 16, 64, {'main': 18432, 'conv16': 36864}),
    (F16, CONV2, 64, 16, {'main': 36864, 'conv16': 36864}),
    (F16, GATE, 64, 16, {'main': 3072, 'gate16': 4096}),
    (F16, CONV, 96, 96, {'main': 165888, 'conv16': 165888}),
    (F16, CONV1, 96, 48, {'main': 110592, 'conv16': 110592, 'conv16t': 82944}),
    (F16, FILM, 96, 96, {'main': 165888, 'conv16': 165888}),
    (F16, CONV, 16, 16, {'main': 9216, 'conv16': 18432}),
    (F16, FILM, 32, 64, {'main': 36864, 'conv16': 36864}),
    (F16, FILM, 48, 96, {'main': 82944, 'conv16': 110592}),
    # f32
    (F32, CONV1, 96, 192, {'main': 663552}),
    (F32, CONV2, 192, 96, {'main': 663552}),
    (F32, GATE, 192, 96, {'main': 73728}),
    (F32, CONV1, 192, 384, {'main': 2654208}),
    (F32, CONV2, 384, 192, {'main': 2654208}),
    (F32, MIX, 384, 192, {'main': 294912}),
    (F32, CONV1, 384, 768, {'main': 10616832}),
    (F32, CONV2, 768, 384, {'main': 10616832}),
    (F32, MIX, 768, 384, {'main': 1179648}),
    (F32, CONV1, 768, 1536, {'main': 42467328}),
    (F32, CONV2, 1536, 768, {'main': 42467328}),
    (F32, MIX, 1536, 768, {'main': 4718592}),
    (F32, QA, 768, 3, {'main': 884736}),
    (F32, UP, 768, 1536, {'main': 42467328}),
    (F32, UP, 384, 768, {'main': 10616832}),
    (F32, UP, 192, 384, {'main': 2654208}),
    (F32, MIX, 192, 96, {'main': 73728}),
    (F32, UP, 96, 384, {'main': 1327104}),
    (F32, HEAD, 96, 12, {'main': 110592}),
    (F32, CONV1, 48, 96, {'main': 165888}),
    (F32, CONV2, 96, 48, {'main': 221184}),
    (F32, GATE, 96, 48, {'main': 28672}),
    (F32, QA, 384, 3, {'main': 442368}),
    (F32, UP, 96, 192, {'main': 663552}),
    (F32, MIX, 96, 48, {'main': 24576}),
    (F32, HEAD, 48, 12, {'main': 55296}),
    (F32, CONV1, 16, 32, {'main': 18432}),
    (F32, CONV2, 32, 16, {'main': 36864}),
    (F32, GATE, 32, 16, {'main': 6144}),
    (F32, CONV1, 32, 64, {'main': 73728}),
    (F32, CONV2, 64, 32, {'main': 73728}),
    (F32, GATE, 64, 32, {'main': 8192}),
    (F32, CONV1, 64, 128, {'main': 294912}),
    (F32, CONV2, 128, 64, {'main': 294912}),
    (F32, GATE, 128, 64, {'main': 32768}),
    (F32, CONV1, 128, 256, {'main': 1179648}),
    (F32, CONV2, 256, 128, {'main': 1179648}),
    (F32, MIX, 256, 128, {'main': 131072}),
    (F32, QA, 128, 3, {'main': 147456}),
    (F32, UP, 128, 256, {'main': 1179648}),
    (F32, MIX, 128, 64, {'main': 32768}),
    (F32, UP, 64, 128, {'main': 294912}),
    (F32, MIX, 64, 32, {'main': 8192}),
    (F32, UP, 32, 64, {'main': 73728}),
    (F32, MIX, 32, 16, {'main': 4096}),
    (F32, UP, 16, 64, {'main': 36864}),
    (F32, HEAD, 16, 12, {'main': 18432}),
    (F32, CONV1, 24, 48, {'main': 73728}),
    (F32, CONV2, 48, 24, {'main': 55296}),
    (F32, GATE, 48, 24, {'main': 8192}),
    (F32, CONV1, 40, 80, {'main': 165888}),
    (F32, CONV2, 80, 40, {'main': 184320}),
    (F32, GATE, 80, 40, {'main': 28672}),
    (F32, CONV1, 72, 144, {'main': 460800}),
    (F32, CONV2, 144, 72, {'main': 497664}),
    (F32, GATE, 144, 72, {'main': 67584}),
    (F32, CONV1, 136, 272, {'main': 1492992}),
    (F32, CONV2, 272, 136, {'main': 1566720}),
    (F32, MIX, 272, 136, {'main': 184320}),
    (F32, QA, 136, 3, {'main': 165888}),
    (F32, UP, 136, 288, {'main': 1658880}),
    (F32, MIX, 144, 72, {'main': 61440}),
    (F32, UP, 72, 160, {'main': 552960}),
    (F32, MIX, 80, 40, {'main': 24576}),
    (F32, UP, 40, 96, {'main': 221184}),
    (F32, MIX, 48, 24, {'main': 8192}),
    (F32, UP, 24, 96, {'main': 147456}),
    (F32, HEAD, 24, 12, {'main': 36864}),
    (F32, CONV1, 256, 512, {'main': 4718592}),
    (F32, CONV2, 512, 256, {'main': 4718592}),
    (F32, MIX, 512, 256, {'main': 524288}),
    (F32, QA, 256, 3, {'main': 294912}),
    (F32, UP, 256, 512, {'main': 4718592}),
    (F32, UP, 32, 128, {'main': 147456}),
    (F32, HEAD, 32, 12, {'main': 36864}),
    (F32, CONV2, 16, 16, {'main': 18432}),
    (F32, GATE, 16, 16, {'main': 6144}),
    (F32, CONV1, 16, 64, {'main': 36864}),
    (F32, CONV2, 64, 16, {'main': 73728}),
    (F32, GATE, 64, 16, {'main': 6144}),
    (F32, CONV, 96, 96, {'main': 331776}),
    (F32, CONV1, 96, 48, {'main': 221184}),
    (F32, FILM, 96, 96, {'main': 331776}),
    (F32, CONV, 16, 16, {'main': 18432}),
    (F32, FILM, 32, 64, {'main': 73728}),
    (F32, FILM, 48, 96, {'main': 165888}),
]


def _lib():
    return _ffi.lib()


def _weights(op, cin, cout):
    return 2 * cout * cout if op in (MIX, GATE) else 9 * cin * cout


def _id(row):
    names = {F32: "F32", BF16: "BF16", F16: "F16"}
    ops = ("CONV1", "CONV", "UP", "HEAD", "QA", "FILM", "CONV2", "MIX", "GATE")
    return f"{names[row[0]]}-{ops[row[1]]}-{row[2]}-{row[3]}"


@pytest.mark.parametrize("row", TABLE, ids=_id)
def test_layout_sets_and_sizes(row):
    dtype, op, cin, cout, want = row
    lib = _lib()
    got = {}
    for i, name in enumerate(LAYOUTS):
        n = lib.mz_debug_pack(dtype, op, cin, cout, i, None, 0)
        if n >= 0:
            got[name] = n * (4 if dtype == F32 else 2)
        else:
            assert b"no packing" in lib.mz_last_error()
    assert got == want


@pytest.mark.parametrize("row", TABLE, ids=_id)
def test_every_weight_packed_once(row):
    dtype, op, cin, cout, want = row
    lib = _lib()
    nw = _weights(op, cin, cout)
    for name, nbytes in want.items():
        n = nbytes // (4 if dtype == F32 else 2)
        src = np.full(n, -2, dtype=np.int64)
        assert lib.mz_debug_pack(dtype, op, cin, cout, LAYOUTS.index(name), src.ctypes.data, n) == n
        real = src[src >= 0]
        assert np.all(src[src < 0] == -1), name
        assert len(real) == nw and np.array_equal(np.bincount(real, minlength=nw), np.ones(nw, dtype=np.int64)), name


def test_table_reaches_every_layout():
    assert {name for r in TABLE for name in r[4]} == set(LAYOUTS)


def test_refusals():
    lib = _lib()
    assert lib.mz_debug_pack(F32, CONV1, 96, 192, LAYOUTS.index("conv16"), None, 0) < 0  # fp32 packs for the 32x32 MFMA only
    assert b"no packing" in lib.mz_last_error()
    assert lib.mz_debug_pack(BF16, GATE, 384, 192, 0, None, 0) < 0  # a 192-channel conv2 does not fuse the mix
    assert b"does not fuse" in lib.mz_last_error()
    assert lib.mz_debug_pack(BF16, MIX, 96, 96, 0, None, 0) < 0
    assert b"cin = 2 cout" in lib.mz_last_error()
    assert lib.mz_debug_pack(BF16, 9, 96, 96, 0, None, 0) < 0
    assert b"bad op" in lib.mz_last_error()
    assert lib.mz_debug_pack(BF16, CONV, 96, 96, len(LAYOUTS), None, 0) < 0
