# The translation units of libmewzoom_hip.so; build.sh and tools/build_variant.sh source this list.
kernel_units=(mz_kernels mz_conv32 mz_conv3s mz_mix16 mz_conv3r mz_conv3t mz_metrics mz_resize mz_interp mz_degrade mz_dihedral mz_color mz_yuv mz_ycbcr mz_alpha mz_feather mz_probe)  # <unit>.hip: -O3, gfx950
host_units=(mz_host mz_ops mz_image mz_debug)  # <unit>.cpp: -O2
