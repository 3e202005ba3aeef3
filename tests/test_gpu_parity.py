"""GPU parity tests: the HIP ELBO engine (through the C-ABI) against the fp64 CPU oracle on identical inputs and
identical injected Monte-Carlo noise.  Tolerance per BASELINE.json north_star: index gathers bit-exact, ELBO and
gradients within 1e-4 relative (fp32 engine vs fp64 oracle)."""
import os

import numpy as np
import pytest
import torch

from oracle import elbo_oracle as O
from tests import util

pytestmark = pytest.mark.gpu

RTOL_LOSS = 1e-4       # north_star tolerance on the ELBO
RTOL_GRAD = 2e-4       # tensor-level (max-norm) relative tolerance on every gradient tensor

CASES = {
    "mlp2x32_normal_img_S3": dict(N=300, R=40, d0=5, L=2, w=32, S=3),
    "mlp5x64_studentt_posenc_S8": dict(N=1000, R=64, d0=5, posenc=True, L=5, w=64, S=8, likelihood="studentt", dof=4.0,
                                       outliers=True),
    "mlp5x64_normal_S1_noimg": dict(N=513, R=33, d0=5, L=5, w=64, S=1, use_image_scales=False),
    "mlp3x20_softplus_shift_S2": dict(N=257, R=50, d0=6, L=3, w=20, S=2, bijector="softplus", shift=3.5),
    "mlp1x64_d40_S1": dict(N=200, R=17, d0=40, L=1, w=64, S=1),
    "mlp4x48_klweight_S4": dict(N=640, R=100, d0=5, L=4, w=48, S=4, kl_weight=0.5, likelihood="studentt", dof=12.0),
    "cli_default_20x10_S1": dict(N=500, R=50, d0=5, L=20, w=10, S=1, perturb=0.02),
    # few persistent workgroups -> each walks several tiles: accumulators (registers, and LDS slots for the upper layers of the
    # narrow kernel) carry over from tile to tile
    "cli_default_20x10_six_tiles_per_workgroup": dict(N=1500, R=60, d0=5, L=20, w=10, S=2, perturb=0.02, grid=2),
    "mlp5x64_five_tiles_per_workgroup": dict(N=1900, R=64, d0=5, L=5, w=64, S=2, grid=3),
    "mlp14x15_d21_S3": dict(N=700, R=30, d0=5, posenc=True, L=14, w=15, S=3, perturb=0.02, grid=2),
    "mlp2x32_S12_studentt": dict(N=300, R=40, d0=5, L=2, w=32, S=12, likelihood="studentt", dof=8.0),       # more than 8 MC samples
    "laue_2x32_S11": dict(N=400, R=40, L=2, w=32, S=11, laue=True),
    # narrow instance, all three MFMA-step counts (hidden width <= 8 / <= 12 / <= 15)
    "mlp9x7_d6_S2": dict(N=700, R=40, d0=6, L=9, w=7, S=2, perturb=0.03, grid=2),         # (since round 6 on the lane kernel's depth-9 instance: widths 7 .. 10 at any depth)
    "narrow_9x4_d6_S2": dict(N=700, R=40, d0=6, L=9, w=4, S=2, perturb=0.03, grid=2),     # ... the narrow kernel's two-step instance keeps widths <= 4
    "lane_depth12_studentt_12x10_d12_S3": dict(N=800, R=50, d0=12, L=12, w=10, S=3, likelihood="studentt", dof=6.0, perturb=0.03, grid=2),
    "lane_depth2_2x9_S2": dict(N=500, R=40, d0=5, L=2, w=9, S=2, perturb=0.05),
    "lane_depth19_19x8_S1": dict(N=600, R=40, d0=7, L=19, w=8, S=1, perturb=0.02, grid=2),
    "lane_depth10_laue_single_pass_10x10_S3": dict(N=900, R=40, L=10, w=10, S=3, laue=True, perturb=0.03, grid=2),
    "mlp7x12_S3_studentt": dict(N=500, R=40, d0=5, L=7, w=12, S=3, likelihood="studentt", dof=6.0, perturb=0.03),
    "mlp5x13_softplus": dict(N=400, R=30, d0=5, L=5, w=13, S=2, bijector="softplus", shift=1.5, perturb=0.03),
    # the narrow kernel (csrc/elbo_narrow.hip: width <= 15, metadata <= 15 columns, plain mono layout) beyond the CLI default
    "narrow_ev11_studentt_6x10_S5": dict(N=700, R=50, d0=5, L=6, w=10, S=5, ev11=True, likelihood="studentt", dof=6.0, perturb=0.03),
    "narrow_klweight_4x10_S12_noimg": dict(N=500, R=40, d0=5, L=4, w=10, S=12, kl_weight=0.5, use_image_scales=False, perturb=0.03),
    "narrow_rows_in_arbitrary_order_S3": dict(N=900, R=60, d0=5, L=5, w=10, S=3, n_images=9, shuffle_rows=True, perturb=0.03),
    "narrow_three_observations": dict(N=3, R=2, d0=5, L=3, w=10, S=2, n_images=1, use_image_scales=False, perturb=0.03),
    "narrow_one_layer_w15_d15_softplus": dict(N=333, R=30, d0=15, L=1, w=15, S=2, bijector="softplus", shift=0.5, perturb=0.03),
    "narrow_20x4_d12": dict(N=600, R=40, d0=12, L=20, w=4, S=1, perturb=0.03, grid=2),
    # the lane-per-observation kernel (csrc/elbo_lane.hip: 20 layers, width <= 10, <= 15 metadata columns, <= 8 MC samples; compile-time widths
    # 4 / 6 / 8 / 10 x metadata capacities 8 / 15) beyond the CLI-default cases above; other depths of the same widths run on the narrow kernel
    "lane_ev11_studentt_20x10_S2": dict(N=700, R=50, d0=5, L=20, w=10, S=2, ev11=True, likelihood="studentt", dof=6.0, perturb=0.02),
    "lane_rows_in_arbitrary_order_20x7_S1": dict(N=900, R=60, d0=5, L=20, w=7, S=1, n_images=9, shuffle_rows=True, perturb=0.02),
    "lane_softplus_shift_20x5_d9_S3": dict(N=400, R=30, d0=9, L=20, w=5, S=3, bijector="softplus", shift=1.5, perturb=0.02),
    "lane_studentt_20x10_S8": dict(N=700, R=50, d0=5, L=20, w=10, S=8, likelihood="studentt", dof=6.0, perturb=0.02, grid=2),
    "lane_normal_20x10_S5_noimg": dict(N=500, R=40, d0=7, L=20, w=10, S=5, use_image_scales=False, perturb=0.02),
    "lane_laue_single_pass_20x10_S7": dict(N=900, R=40, L=20, w=10, S=7, laue=True, perturb=0.02, grid=2),
    "lane_klweight_20x3_S2_noimg": dict(N=500, R=40, d0=5, L=20, w=3, S=2, kl_weight=0.5, use_image_scales=False, perturb=0.02),
    "lane_20x10_d12_S2": dict(N=600, R=40, d0=12, L=20, w=10, S=2, perturb=0.02),
    "lane_20x8_d15_S1_studentt": dict(N=700, R=40, d0=15, L=20, w=8, S=1, likelihood="studentt", dof=5.0, perturb=0.02, grid=2),
    "lane_20x6_S2": dict(N=1300, R=60, d0=6, L=20, w=6, S=2, perturb=0.02, grid=2),
    "lane_20x9_d1_three_observations": dict(N=3, R=2, d0=1, L=20, w=9, S=1, n_images=1, use_image_scales=False, perturb=0.02),
    "lane_laue_single_pass_20x10_S2": dict(N=900, R=40, L=20, w=10, S=2, laue=True, perturb=0.02, grid=2),
    "lane_laue_single_pass_20x6_S1_ev11": dict(N=600, R=40, L=20, w=6, S=1, laue=True, ev11=True, perturb=0.02),
    "lane_laue_image_layers2_peeled_d21_S2": dict(N=900, R=40, L=20, w=10, S=2, laue=True, image_layers=2, n_images=7, extra_meta=15, perturb=0.02),   # (round 6: Laue + per-image layers behind the peeled first layer)
    # ... with 16 .. 31 metadata columns (positional encodings: + 16 columns; the rows of a tile then live in LDS, layer 0 has two
    # input blocks) and with more than eight MC samples (batches of eight through LDS)
    "lane_20x10_d21_S8_studentt": dict(N=900, R=50, d0=5, posenc=True, L=20, w=10, S=8, likelihood="studentt", dof=16.0, outliers=True, perturb=0.02, grid=2),
    "lane_20x10_d31_S3": dict(N=700, R=40, d0=31, L=20, w=10, S=3, perturb=0.02, grid=2),
    "lane_20x10_d16_S1_softplus": dict(N=500, R=40, d0=16, L=20, w=10, S=1, bijector="softplus", shift=1.5, perturb=0.02),
    "lane_20x4_d29_S2_ev11": dict(N=333, R=30, d0=29, L=20, w=4, S=2, ev11=True, perturb=0.02),
    "lane_20x7_d24_S12_klweight": dict(N=600, R=40, d0=24, L=20, w=7, S=12, kl_weight=0.5, likelihood="studentt", dof=8.0, perturb=0.02),
    "lane_20x10_S12": dict(N=500, R=40, d0=5, L=20, w=10, S=12, perturb=0.02),
    "lane_20x10_S17_studentt_noimg": dict(N=300, R=30, d0=9, L=20, w=10, S=17, likelihood="studentt", dof=6.0, use_image_scales=False, perturb=0.02),
    "lane_laue_single_pass_20x10_S11": dict(N=700, R=40, L=20, w=10, S=11, laue=True, perturb=0.02, grid=2),
    "lane_laue_single_pass_20x8_d22_S3": dict(N=900, R=40, L=20, w=8, S=3, laue=True, extra_meta=16, perturb=0.02, grid=2),
    "lane_d21_three_observations": dict(N=3, R=2, d0=21, L=20, w=10, S=2, n_images=1, use_image_scales=False, perturb=0.02),
    # ... with MORE than 31 metadata columns (round 5: four positionally encoded keys give 37): the first layer is peeled -- its
    # pre-activations and its weight gradient come from csrc/elbo_peel.hip, the lane kernel runs the scaler with an identity first layer
    "peel_20x10_d37_S1": dict(N=900, R=50, d0=37, L=20, w=10, S=1, perturb=0.02, grid=2),
    "peel_20x10_d53_S8_studentt": dict(N=1100, R=50, d0=53, L=20, w=10, S=8, likelihood="studentt", dof=16.0, outliers=True, perturb=0.02, grid=2),
    "peel_20x6_d64_S2_softplus_ev11": dict(N=600, R=40, d0=64, L=20, w=6, S=2, bijector="softplus", shift=1.5, ev11=True, perturb=0.02),
    "peel_20x10_d32_S3_klweight_noimg": dict(N=500, R=40, d0=32, L=20, w=10, S=3, kl_weight=0.5, use_image_scales=False, perturb=0.02),
    "peel_laue_single_pass_20x8_d38_S3": dict(N=900, R=40, L=20, w=8, S=3, laue=True, extra_meta=32, perturb=0.02, grid=2),
    "peel_double_wilson_20x10_d40_S2": dict(N=600, R=60, d0=40, L=20, w=10, S=2, double_wilson=True, perturb=0.02),
    "peel_rows_in_arbitrary_order_20x10_d37": dict(N=900, R=60, d0=37, L=20, w=10, S=2, n_images=9, shuffle_rows=True, perturb=0.02),
    # ... and the same in front of the narrow kernel (any depth <= 20, hidden width <= 15, more than 15 columns)
    "peel_narrow_7x12_d21_S2": dict(N=700, R=40, d0=5, posenc=True, L=7, w=12, S=2, perturb=0.03, grid=2),
    "peel_narrow_20x15_d40_S3_studentt": dict(N=600, R=40, d0=40, L=20, w=15, S=3, likelihood="studentt", dof=8.0, perturb=0.02),
    "peel_narrow_1x9_d16": dict(N=333, R=30, d0=16, L=1, w=9, S=1, perturb=0.03),
    "peel_narrow_laue_single_pass_5x10_d22_ev11": dict(N=800, R=40, L=5, w=10, S=2, laue=True, extra_meta=16, ev11=True, perturb=0.03, grid=2),
    "peel_narrow_12x13_d64_klweight": dict(N=500, R=40, d0=64, L=12, w=13, S=2, kl_weight=0.5, perturb=0.03),
    "peel_d45_three_observations": dict(N=3, R=2, d0=45, L=20, w=10, S=2, n_images=1, use_image_scales=False, perturb=0.02),
    "narrow_one_layer_w9_d1": dict(N=333, R=30, d0=1, L=1, w=9, S=1, perturb=0.03),
    "narrow_laue_single_pass_7x6_S1_ev11": dict(N=600, R=40, L=7, w=6, S=1, laue=True, ev11=True, perturb=0.03),
    "image_layers2_3x8": dict(N=800, R=40, d0=5, L=3, w=8, S=2, n_images=5, image_layers=2, perturb=0.03),
    "laue_two_pass_narrow_8x5": dict(N=500, R=40, L=8, w=5, S=2, laue=True, two_pass=True, perturb=0.03),
    "mlp8x24_S2_studentt": dict(N=300, R=30, d0=5, L=8, w=24, S=2, likelihood="studentt", dof=4.0, perturb=0.03),
    "mlp12x16_d21_S3": dict(N=260, R=30, d0=5, posenc=True, L=12, w=16, S=3, perturb=0.02),
    # width EXACTLY 16 (round 5): the 16-wide instance without the constant-one feature (slot 15 is feature 15, explicit bias gradient), up to
    # 20 layers in one launch -- it used to pad to the 32-wide instance
    "w16_20x16_S2_studentt": dict(N=700, R=40, d0=5, L=20, w=16, S=2, likelihood="studentt", dof=8.0, perturb=0.02, grid=2),
    "w16_3x16_d40_S1_softplus_ev11": dict(N=500, R=40, d0=40, L=3, w=16, S=1, bijector="softplus", shift=0.5, ev11=True, perturb=0.03),
    "w16_laue_single_pass_8x16_S3": dict(N=800, R=40, L=8, w=16, S=3, laue=True, perturb=0.03, grid=2),
    "w16_laue_two_pass_5x16": dict(N=500, R=40, L=5, w=16, S=2, laue=True, two_pass=True, perturb=0.03),
    "w16_deep_25x16_klweight": dict(N=500, R=40, d0=5, L=25, w=16, S=2, kl_weight=0.5, perturb=0.02),
    "w16_double_wilson_6x16_d9": dict(N=400, R=60, d0=9, L=6, w=16, S=2, double_wilson=True, perturb=0.03),
    "w16_image_layers1_3x16": dict(N=700, R=40, d0=5, L=3, w=16, S=2, n_images=5, image_layers=1, perturb=0.03),
    "ev11_normal_2x32_S3": dict(N=400, R=40, d0=5, L=2, w=32, S=3, ev11=True),
    "ev11_studentt_5x64_S8": dict(N=500, R=50, d0=5, L=5, w=64, S=8, ev11=True, likelihood="studentt", dof=8.0),
    "ev11_laue_normal_2x32_S2": dict(N=400, R=40, L=2, w=32, S=2, laue=True, ev11=True),
    "laue_2x32_normal_S3": dict(N=400, R=40, L=2, w=32, S=3, laue=True),
    "laue_5x64_studentt_S2_noimg": dict(N=700, R=64, L=5, w=64, S=2, laue=True, likelihood="studentt", dof=6.0, use_image_scales=False),
    "double_wilson_2x32_S3": dict(N=400, R=60, d0=5, L=2, w=32, S=3, double_wilson=True),
    # --image-layers: NeuralImageScaler (per-image kernels after the Dense stack); images of very different sizes, > 1 tile
    "image_layers1_2x32_S3": dict(N=700, R=40, d0=5, L=2, w=32, S=3, n_images=5, image_layers=1),
    "image_layers2_3x64_S8_studentt": dict(N=1500, R=64, d0=5, posenc=True, L=3, w=64, S=8, n_images=7, image_layers=2,
                                           likelihood="studentt", dof=16.0),
    "image_layers2_4x10_softplus": dict(N=900, R=50, d0=5, L=4, w=10, S=2, n_images=6, image_layers=2, bijector="softplus",
                                        shift=0.7),
    "image_layers2_on_the_cli_default_20x10": dict(N=600, R=40, d0=5, L=20, w=10, S=2, n_images=4, image_layers=2),
    # `--image-layers 1|2` on the default scaler: the lane-per-observation kernel with per-image top layers (elbo_lane.hip, round 5);
    # many images per wave (flush + reload at every change), a narrower scaler on the widest instance, 12 columns (DMAX = 15), two
    # sample batches, the Evans-2011 error model, Student-T
    "lane_image_layers1_20x10_many_images": dict(N=3000, R=120, d0=5, L=20, w=10, S=1, n_images=37, image_layers=1, perturb=0.03),
    "lane_image_layers2_20x8_d12_S3_studentt": dict(N=1500, R=80, d0=12, L=20, w=8, S=3, n_images=9, image_layers=2, likelihood="studentt", dof=8.0,
                                                    perturb=0.03),
    "lane_image_layers2_20x10_S11_softplus": dict(N=900, R=50, d0=5, L=20, w=10, S=11, n_images=6, image_layers=2, bijector="softplus", perturb=0.03),
    "lane_image_layers1_20x6_ev11": dict(N=800, R=50, d0=7, L=20, w=6, S=2, n_images=5, image_layers=1, ev11=True, perturb=0.03),
    # ... on more than the 15 columns the lane instances hold: the first layer peeled in front of them (`--image-layers 2 --positional-encoding-keys X,Y`)
    "lane_image_layers2_20x10_posenc_d21_peeled": dict(N=1500, R=60, d0=5, posenc=True, L=20, w=10, S=2, n_images=8, image_layers=2, perturb=0.03),
    "lane_image_layers1_20x8_d30_peeled_studentt_S9": dict(N=1200, R=50, d0=30, L=20, w=8, S=9, n_images=11, image_layers=1, likelihood="studentt", dof=8.0,
                                                           perturb=0.03),
    "lane_laue_image_layers1_20x10": dict(N=900, R=60, L=20, w=10, S=1, laue=True, n_images=6, image_layers=1, perturb=0.03),
    "lane_laue_image_layers2_20x6_S3_studentt": dict(N=700, R=50, L=20, w=6, S=3, laue=True, n_images=4, image_layers=2, likelihood="studentt", dof=8.0,
                                                     perturb=0.03),
    # per-image layers at hidden width <= 15 on MORE THAN 32 columns: the 32-wide instance (round 6: the 16-wide <16, 64, 24> instance faulted when a
    # workgroup crossed an image border -- the first case is the random draw that found it), deeper than it holds: layer by layer
    "image_layers2_2x11_d36_workgroups_cross_images": dict(N=323, R=67, L=2, w=11, S=7, perturb=0.05, d0=36, image_layers=2, n_images=7, bijector="softplus", shift=0.0, grid=2),
    "image_layers2_2x15_d36_one_workgroup": dict(N=323, R=67, L=2, w=15, S=2, perturb=0.05, d0=36, image_layers=2, n_images=3, grid=1),
    "image_layers1_8x13_d50_S3_studentt": dict(N=900, R=60, L=8, w=13, S=3, perturb=0.03, d0=50, image_layers=1, n_images=6, likelihood="studentt", dof=8.0, grid=3),
    "image_layers1_12x12_d36_layer_by_layer": dict(N=700, R=50, d0=36, L=12, w=12, S=2, n_images=5, image_layers=1, perturb=0.02),
    # three per-image layers on the default depth (round 6: a lane unit of their own)
    "lane_image_layers3_20x10": dict(N=1500, R=60, d0=5, L=20, w=10, S=2, n_images=9, image_layers=3, perturb=0.02),
    "lane_image_layers3_20x7_d12_ev11_studentt_S5": dict(N=1200, R=60, d0=12, L=20, w=7, S=5, n_images=7, image_layers=3, ev11=True, likelihood="studentt", dof=8.0, perturb=0.02),
    "lane_image_layers3_20x10_posenc_d21_peeled": dict(N=1500, R=60, d0=5, posenc=True, L=20, w=10, S=2, n_images=8, image_layers=3, perturb=0.02),
    "lane_laue_image_layers3_20x10_S3": dict(N=900, R=60, L=20, w=10, S=3, laue=True, n_images=6, image_layers=3, perturb=0.02),
    # ... at other depths (round 6: the per-depth units' per-image-layer instances)
    "lane_image_layers3_10x10": dict(N=1500, R=60, d0=5, L=10, w=10, S=2, n_images=9, image_layers=3, perturb=0.03),
    "lane_image_layers3_2x8_ev11": dict(N=900, R=50, d0=9, L=2, w=8, S=3, n_images=6, image_layers=3, ev11=True, perturb=0.04),
    "lane_image_layers3_18x10_studentt": dict(N=1200, R=60, d0=5, L=18, w=10, S=2, n_images=7, image_layers=3, likelihood="studentt", dof=8.0, perturb=0.02),
    "lane_image_layers3_7x10_posenc_d21_peeled": dict(N=1500, R=60, d0=5, posenc=True, L=7, w=10, S=2, n_images=8, image_layers=3, perturb=0.03),
    "lane_laue_image_layers3_14x9": dict(N=900, R=60, L=14, w=9, S=2, laue=True, n_images=6, image_layers=3, perturb=0.02),
    "lane_image_layers2_10x10": dict(N=1500, R=60, d0=5, L=10, w=10, S=2, n_images=9, image_layers=2, perturb=0.03),
    "lane_image_layers1_2x10_S3": dict(N=900, R=50, d0=5, L=2, w=10, S=3, n_images=6, image_layers=1, perturb=0.04),
    "lane_image_layers2_2x6_d12": dict(N=900, R=50, d0=12, L=2, w=6, S=2, n_images=6, image_layers=2, perturb=0.04),
    "lane_image_layers2_19x9_ev11_studentt": dict(N=1200, R=60, d0=7, L=19, w=9, S=2, n_images=7, image_layers=2, ev11=True, likelihood="studentt", dof=8.0, perturb=0.02),
    "lane_image_layers2_12x10_posenc_d21_peeled": dict(N=1500, R=60, d0=5, posenc=True, L=12, w=10, S=2, n_images=8, image_layers=2, perturb=0.03),
    "lane_laue_image_layers2_8x10_S3": dict(N=900, R=60, L=8, w=10, S=3, laue=True, n_images=6, image_layers=2, perturb=0.03),
    "lane_laue_image_layers1_15x7_peeled_d21": dict(N=900, R=40, L=15, w=7, S=2, laue=True, image_layers=1, n_images=7, extra_meta=15, perturb=0.02),
    "lane_image_layers2_20x10_rows_in_arbitrary_order": dict(N=1200, R=60, d0=5, L=20, w=10, S=2, n_images=11, image_layers=2, shuffle_rows=True,
                                                             perturb=0.03),
    "laue_image_layers1_2x32": dict(N=600, R=60, L=2, w=32, S=3, laue=True, n_images=4, image_layers=1),
    # the two Laue code paths: single pass (group sums inside the fused kernel; the default) and two passes around the group sums
    "laue_two_pass_2x32_S3": dict(N=400, R=40, L=2, w=32, S=3, laue=True, two_pass=True),
    "laue_two_pass_ev11_studentt_S5": dict(N=500, R=40, L=2, w=32, S=5, laue=True, ev11=True, likelihood="studentt", dof=6.0, two_pass=True),
    "laue_two_pass_image_layers1": dict(N=600, R=60, L=2, w=32, S=3, laue=True, n_images=4, image_layers=1, two_pass=True),
    # (two-pass Laue, per-image layers, more than 32 columns: cl_mlp_backward_ext has no route for 20 + 2 layers there -- layer by layer)
    "laue_two_pass_image_layers2_20x10_d36": dict(N=600, R=40, L=20, w=10, S=2, laue=True, n_images=5, image_layers=2, extra_meta=30, two_pass=True,
                                                  perturb=0.02),
    "laue_two_pass_narrow_12x10": dict(N=600, R=40, L=12, w=10, S=2, laue=True, two_pass=True, perturb=0.02),
    "laue_single_pass_narrow_20x10": dict(N=900, R=40, L=20, w=10, S=3, laue=True, perturb=0.02, grid=2),
    "laue_ev11_studentt_S5": dict(N=500, R=40, L=2, w=32, S=5, laue=True, ev11=True, likelihood="studentt", dof=6.0),
    "laue_groups_up_to_12_rows_S6": dict(N=700, R=50, L=2, w=32, S=6, laue=True, regroup=4),
    "laue_groups_over_16_rows_fall_back": dict(N=700, R=50, L=2, w=32, S=2, laue=True, regroup=16),
    "mono_rows_in_arbitrary_order_S5": dict(N=900, R=60, d0=5, L=3, w=64, S=5, n_images=9, shuffle_rows=True, likelihood="studentt", dof=4.0),
    "mono_three_observations": dict(N=3, R=2, d0=5, L=2, w=32, S=2, n_images=1, use_image_scales=False),
    # scalers deeper than one launch holds: chains of layer blocks (activations through HBM, forward recomputed per block)
    "deep_12x64_studentt_S4": dict(N=700, R=50, d0=5, posenc=True, L=12, w=64, S=4, likelihood="studentt", dof=8.0),
    "deep_25x10_softplus": dict(N=500, R=40, d0=5, L=25, w=10, S=2, bijector="softplus", shift=0.5),
    # (round 6: at width <= 10 the last 20 layers of a chained scaler run on the lane kernel, cl_chain_dx hands dZ_0 back as the gradient of the boundary activations)
    "deep_24x10_d12_studentt_S3": dict(N=700, R=40, d0=12, L=24, w=10, S=3, likelihood="studentt", dof=6.0, perturb=0.02, grid=2),
    "deep_45x8_three_blocks": dict(N=500, R=40, d0=5, L=45, w=8, S=2, perturb=0.01),
    "deep_22x6_double_wilson": dict(N=600, R=40, d0=5, L=22, w=6, S=2, double_wilson=True, perturb=0.02),
    "deep_26x12_d9_S2": dict(N=700, R=40, d0=9, L=26, w=12, S=2, perturb=0.01, grid=2),            # widths 11, 12: seven layers in front, nineteen on the twelve-wide lane instance
    "deep_45x11_three_blocks": dict(N=400, R=30, d0=5, L=45, w=11, S=1, perturb=0.01),
    "deep_11x32_noimg": dict(N=400, R=40, d0=5, L=11, w=32, S=3, use_image_scales=False),
    "deep_laue_7x64": dict(N=500, R=50, L=7, w=64, S=2, laue=True, two_pass=True),
    "deep_double_wilson_6x64": dict(N=400, R=60, d0=5, L=6, w=64, S=2, double_wilson=True),
    # hidden / metadata width beyond 64: unfused scaler on the engine's own fp32-MFMA GEMM kernels (csrc/wide_gemm.hip) around the same HIP likelihood kernels
    "wide_3x96_studentt_S3": dict(N=700, R=50, d0=5, L=3, w=96, S=3, likelihood="studentt", dof=6.0),
    "wide_2x128_softplus_noimg": dict(N=400, R=40, d0=5, L=2, w=128, S=2, bijector="softplus", shift=1.5, use_image_scales=False),
    "wide_metadata_d70_2x32": dict(N=300, R=30, d0=70, L=2, w=32, S=2),
    # several workgroups of the square-layer kernels, a ragged last 16-row block, the widest metadata the recomputed first layer takes
    # (8 columns: its weight gradient rides on the second layer's dgrad, round 4), the narrowest width of that kernel (5 blocks of 16)
    "wide_3x128_d8_rows2117_S2": dict(N=2117, R=90, d0=8, L=3, w=128, S=2, likelihood="studentt", dof=10.0),
    "wide_4x72_rows1301_noimg": dict(N=1301, R=70, d0=5, L=4, w=72, S=2, use_image_scales=False),
    "wide_3x96_d15_rows1203": dict(N=1203, R=60, d0=15, L=3, w=96, S=2, likelihood="studentt", dof=8.0),      # (the widest recomputed first layer)
    "wide_2x128_d12": dict(N=900, R=50, d0=12, L=2, w=128, S=3),
    "wide_mono_2x80_ev11_S4": dict(N=600, R=50, d0=5, L=2, w=80, S=4, ev11=True),      # (the Evans-2011 terms of the one-launch slot kernel)
    "wide_laue_2x80_ev11": dict(N=500, R=40, L=2, w=80, S=2, laue=True, ev11=True),
    # the instances no case above reaches (tests/test_wide_kernels.py calls each entry point directly; these run them inside whole steps):
    # widths 97 .. 112 = seven 16-column blocks (wide_sq_kernel<.., 7> in its PRE / WG0 / HEADB / LIK forms, wide_stream2_kernel<7>), 120 = the
    # same with a ragged block, 65 = one column past the fused kernels, 300 / 520 = three / five 128-column tiles and
    # wide_head_backward_kernel<4> / <8>, metadata wider than 128 (K > 128 on the tiled kernel; N <= 64: its 64-column instance) and a
    # non-square first layer on the 8-block streaming instance (100 -> 96)
    "wide_3x100_d8_S2": dict(N=1301, R=70, d0=8, L=3, w=100, S=2, perturb=0.02),
    "wide_3x120_d12_S2_studentt": dict(N=700, R=50, d0=12, L=3, w=120, S=2, likelihood="studentt", dof=8.0, perturb=0.02),
    "wide_3x65_d5": dict(N=700, R=50, d0=5, L=3, w=65, S=3, perturb=0.02),
    "wide_2x300_d5_S2": dict(N=400, R=40, d0=5, L=2, w=300, S=2, perturb=0.02),
    "wide_2x520_S1": dict(N=300, R=30, d0=5, L=2, w=520, S=1, perturb=0.02),
    "wide_metadata_d130_2x32": dict(N=300, R=30, d0=130, L=2, w=32, S=2, perturb=0.02),
    "wide_metadata_d100_3x96": dict(N=500, R=40, d0=100, L=3, w=96, S=2, perturb=0.02),
    "wide_metadata_d200_2x144": dict(N=300, R=30, d0=200, L=2, w=144, S=2, perturb=0.02),
    # per-image layers beyond one fused launch: wider than 64, or more hidden layers (Dense + per-image) than a launch holds at the
    # width -- layer by layer on the grouped GEMM kernels (csrc/wide_gemm.hip), rows stored in image order
    "wide_image_layers1_2x96_S3": dict(N=700, R=40, d0=5, L=2, w=96, S=3, n_images=5, image_layers=1),
    "wide_image_layers2_1x128_studentt_rows_in_arbitrary_order": dict(N=900, R=50, d0=5, L=1, w=128, S=2, n_images=7, image_layers=2, likelihood="studentt",
                                                                      dof=6.0, shuffle_rows=True),
    # per-image layers wider than 128 (round 4: the tiled kernel over a list of (image, 128-row piece) blocks; the reference has no limit)
    "wide_image_layers2_2x144_S2": dict(N=900, R=40, d0=5, L=2, w=144, S=2, n_images=6, image_layers=2, perturb=0.03),
    "wide_laue_image_layers1_1x160_studentt": dict(N=500, R=40, L=1, w=160, S=2, laue=True, n_images=4, image_layers=1, likelihood="studentt", dof=8.0,
                                                   perturb=0.03),
    # more images than the grouped kernels have workgroups (2 CUs): a workgroup takes a second image (`grp += gridDim.x`); the count is
    # fixed at collection (2 * 256 + 48) so the case list does not depend on the device
    "wide_image_layers1_2x72_many_images": dict(N=1400, R=60, d0=5, L=2, w=72, S=2, n_images=2 * 256 + 48, image_layers=1, perturb=0.02),
    "deep_image_layers2_5x64_S2": dict(N=800, R=40, d0=5, L=5, w=64, S=2, n_images=6, image_layers=2),
    "deep_image_layers3_9x32_softplus": dict(N=600, R=40, d0=5, L=9, w=32, S=2, n_images=4, image_layers=3, bijector="softplus", shift=0.5, perturb=0.03),
    "wide_laue_image_layers1_2x80": dict(N=600, R=50, L=2, w=80, S=2, laue=True, n_images=4, image_layers=1),
    "double_wilson_trainable_r_S4": dict(N=400, R=60, d0=5, L=2, w=32, S=4, double_wilson=True, optimize_dw_r=True),
    "double_wilson_5x64_S8_studentt": dict(N=600, R=80, d0=5, L=5, w=64, S=8, double_wilson=True, likelihood="studentt", dof=8.0),
}


def _regroup_laue(data, div):
    """Merge every `div` consecutive harmonic groups into one (bigger groups than the generator makes)."""
    hid = np.asarray(data["harmonic_id"]) // div
    G = int(hid.max()) + 1
    N = len(hid)
    rng = np.random.default_rng(5)
    iobs = np.ones(N, dtype=np.float32); sig = np.ones(N, dtype=np.float32)
    iobs[:G] = (np.bincount(hid, weights=np.maximum(np.asarray(data["iobs"])[: len(hid)], 0.0), minlength=G)[:G] + rng.normal(size=G)).astype(np.float32)
    sig[:G] = np.sqrt(np.abs(iobs[:G]) + 25.0)
    data = dict(data)
    data["harmonic_id"], data["iobs"], data["sigiobs"], data["n_groups"] = hid.astype(np.int64), iobs, sig, G
    return data


def _run_case(kw):
    kw = dict(kw)
    two_pass, regroup, shuffle = kw.pop("two_pass", False), kw.pop("regroup", 0), kw.pop("shuffle_rows", False)
    grid = kw.pop("grid", None)
    L, w = kw["L"], kw["w"]
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    if regroup:
        data = _regroup_laue(data, regroup)
        x = O.inputs_from_numpy(data)
    if shuffle:                                   # rows in arbitrary order: image ids unsorted inside a wave (per-lane atomics path)
        perm = np.random.default_rng(2).permutation(kw["N"])
        for k in ("refl_id", "image_id", "file_id", "metadata", "iobs", "sigiobs"):
            data[k] = np.asarray(data[k])[perm]
        eta = eta[:, perm]
        x = O.inputs_from_numpy(data)
    out, grads = O.elbo_value_and_grads(params, x, cfg, torch.as_tensor(u_f, dtype=torch.float64),
                                        torch.as_tensor(eta, dtype=torch.float64))
    model = util.build_model(data, cfg, params, L, w)
    model.laue_two_pass = two_pass
    model.kernel_grid = grid
    inputs = util.reference_inputs(data)
    ipred = model(inputs, u_f=u_f, eta=eta)
    eng = model._engine
    if kw.get("laue"):
        biggest = int(np.bincount(np.asarray(data["harmonic_id"])).max())
        assert eng.obs.fused_laue == (not two_pass and biggest <= 16 and not eng.wide)    # groups of more than 16 rows fall back to two passes
        if regroup:
            assert (biggest > 16) == (regroup >= 16)
    torch.cuda.synchronize()
    terms = eng.loss_terms()
    return out, grads, ipred.cpu().numpy(), terms, [g.cpu().numpy() for g in eng.grad_tensors()], eng, (data, cfg, params, u_f, eta)


MAX_FLIP_CANDIDATES = 10     # pre-activations within fp32 rounding of zero that the gate is prepared to resolve (2^k oracle runs at most)
FLIP_CASES = []              # cases that needed a forced branch (reported; test_flip_resolutions_stay_rare bounds their number)


def _assert_grads(g_hip, grads, prob, name=""):
    """Every gradient tensor within RTOL_GRAD (max-norm) of the fp64 oracle -- no looser fallback.

    The one way an exact-fp32 engine legitimately leaves that band: a LeakyReLU pre-activation that lies within the rounding error of
    its fp32 dot product of zero comes out on the other side of zero than in fp64 (in ANY fp32 implementation, the reference's
    included; which side depends on the summation order).  The activation hardly moves, its derivative switches between 1 and the
    leak, and the gradients below that unit move by that one observation's share, O(1 / N).  The gate resolves this EXACTLY: the
    oracle lists the pre-activations inside the rounding bound (`near`), and the fp64 oracle is re-run with subsets of them forced
    onto the other branch (`flips`); the engine must agree with ONE such assignment on EVERY tensor at the full RTOL_GRAD.  A kernel
    bug does not survive this: it would have to equal the effect of flipping a unit that is provably at rounding distance."""
    assert len(g_hip) == len(grads)
    errs = [util.rel_err(a, b.numpy()) for a, b in zip(g_hip, grads)]
    if max(errs) < RTOL_GRAD:
        return
    import itertools
    data, cfg, params, u_f, eta = prob
    x = O.inputs_from_numpy(data)
    u64, e64 = torch.as_tensor(u_f, dtype=torch.float64), torch.as_tensor(eta, dtype=torch.float64)
    near = []
    O.elbo_value_and_grads(params, x, cfg, u64, e64, near=near)
    near.sort()
    cand = [(l, r, u) for _, l, r, u in near[:MAX_FLIP_CANDIDATES]]
    assert cand, f"gradient errors {errs} and no LeakyReLU pre-activation within fp32 rounding of zero: not a branch flip"
    best = (max(errs), ())
    for k in range(1, len(cand) + 1):
        for sub in itertools.combinations(cand, k):
            _, gf = O.elbo_value_and_grads(params, x, cfg, u64, e64, flips=sub)
            e = max(util.rel_err(a, b.numpy()) for a, b in zip(g_hip, gf))
            if e < best[0]:
                best = (e, sub)
            if e < RTOL_GRAD:
                FLIP_CASES.append((name, sub, e))
                # (not a warning: this IS the check passing at full tolerance; `pytest -rP` shows the line, the count is bounded below)
                print(f"{name}: gradients match the fp64 oracle at {e:.1e} with the LeakyReLU unit(s) (layer, row, unit) {list(sub)} on the "
                      f"engine's branch (pre-activation within fp32 rounding of zero; {max(errs):.1e} on the fp64 branch)")
                return
    raise AssertionError(f"gradient errors {errs}; best forced-branch assignment {best[1]} still at {best[0]:.2e} (candidates {cand})")


@pytest.mark.parametrize("name", list(CASES))
def test_loss_and_gradients_match_oracle(name):
    out, grads, ipred, terms, g_hip, eng, prob = _run_case(CASES[name])
    if name == "laue_two_pass_image_layers2_20x10_d36":
        assert eng.d > 32
    assert abs(terms["nll"] - float(out["nll"])) <= RTOL_LOSS * abs(float(out["nll"])), (terms, float(out["nll"]))
    assert abs(terms["kl"] - float(out["kl"])) <= RTOL_LOSS * max(abs(float(out["kl"])), 1.0), (terms, float(out["kl"]))
    assert abs(terms["loss"] - float(out["loss"])) <= RTOL_LOSS * abs(float(out["loss"]))
    assert util.rel_err(ipred, out["ipred"].numpy()) < 1e-4
    assert len(g_hip) == len(grads)
    _assert_grads(g_hip, grads, prob, name)


def _random_lane_cases(n=14, seed=2024):
    """Seeded random draws from the lane-per-observation kernel's support (20 layers, width <= 10, <= 15 metadata columns, <= 8 MC
    samples; csrc/elbo_lane.hip): ragged observation counts, one or several tiles per workgroup, every likelihood / bijector /
    loss-reduction switch, mono and single-pass Laue."""
    rng = np.random.default_rng(seed)
    cases = {}
    for i in range(n):
        laue = bool(i % 5 == 4)
        w = int(rng.integers(1, 11)); S = int(rng.integers(1, 9))
        kw = dict(N=int(rng.integers(3, 1400)), R=int(rng.integers(2, 70)), L=20, w=w, S=S, perturb=0.02)
        if laue:
            kw["laue"] = True
            kw["N"] = max(kw["N"], 100)
        else:
            kw["d0"] = int(rng.integers(1, 16))
            if rng.random() < 0.3:
                kw["shuffle_rows"] = True
                kw["n_images"] = int(rng.integers(1, 12))
        if rng.random() < 0.5:
            kw.update(likelihood="studentt", dof=float(rng.choice([3.0, 8.0, 32.0])))
        if rng.random() < 0.3:
            kw["ev11"] = True
        if rng.random() < 0.3:
            kw.update(bijector="softplus", shift=float(rng.choice([0.0, 1.5])))
        if rng.random() < 0.25:
            kw["kl_weight"] = 0.5
        if rng.random() < 0.3:
            kw["use_image_scales"] = False
        if rng.random() < 0.5:
            kw["grid"] = int(rng.integers(1, 4))
        kw["R"] = min(kw["R"], kw["N"])
        if kw.get("n_images") == 1:
            kw["use_image_scales"] = False        # (one image: no image-scale parameter; the engine then has no such tensor)
        cases[f"lane_random_{i:02d}_20x{w}_S{S}" + ("_laue" if laue else f"_d{kw['d0']}")] = kw
    return cases


def _random_lane_rows_cases(n=8, seed=77):
    """The same for the part of the lane kernel's support that round 3 added: 16 .. 31 metadata columns (rows of an LDS buffer, two
    input blocks of layer 0) and up to 20 MC samples (batches of eight)."""
    rng = np.random.default_rng(seed)
    cases = {}
    for i in range(n):
        laue = bool(i % 4 == 3)
        w = int(rng.integers(1, 11)); S = int(rng.integers(1, 21)); d = int(rng.integers(16, 32))
        kw = dict(N=int(rng.integers(3, 1100)), R=int(rng.integers(2, 60)), L=20, w=w, S=S, perturb=0.02)
        if laue:
            kw.update(laue=True, extra_meta=d - 6)
            kw["N"] = max(kw["N"], 100)
        else:
            kw["d0"] = d
            if rng.random() < 0.3:
                kw["shuffle_rows"] = True
                kw["n_images"] = int(rng.integers(2, 12))
        if rng.random() < 0.5:
            kw.update(likelihood="studentt", dof=float(rng.choice([3.0, 8.0, 32.0])))
        if rng.random() < 0.3:
            kw["ev11"] = True
        if rng.random() < 0.3:
            kw.update(bijector="softplus", shift=float(rng.choice([0.0, 1.5])))
        if rng.random() < 0.25:
            kw["kl_weight"] = 0.5
        if rng.random() < 0.3:
            kw["use_image_scales"] = False
        if rng.random() < 0.5:
            kw["grid"] = int(rng.integers(1, 4))
        kw["R"] = min(kw["R"], kw["N"])
        cases[f"lane_rows_random_{i:02d}_20x{w}_S{S}_d{d}" + ("_laue" if laue else "")] = kw
    return cases


# (a longer sweep on demand: LANE_RANDOM_N=200 LANE_RANDOM_SEED=7 python -m pytest tests/test_gpu_parity.py -k random_shapes)
RANDOM_LANE_CASES = _random_lane_cases(int(os.environ.get("LANE_RANDOM_N", "14")), int(os.environ.get("LANE_RANDOM_SEED", "2024")))
RANDOM_LANE_CASES.update(_random_lane_rows_cases(int(os.environ.get("LANE_ROWS_RANDOM_N", "8")), int(os.environ.get("LANE_ROWS_RANDOM_SEED", "77"))))


@pytest.mark.parametrize("name", list(RANDOM_LANE_CASES))
def test_random_shapes_on_the_lane_kernel(name):
    out, grads, ipred, terms, g_hip, eng, prob = _run_case(RANDOM_LANE_CASES[name])
    assert abs(terms["nll"] - float(out["nll"])) <= RTOL_LOSS * abs(float(out["nll"])), (terms, float(out["nll"]))
    assert abs(terms["kl"] - float(out["kl"])) <= RTOL_LOSS * max(abs(float(out["kl"])), 1.0), (terms, float(out["kl"]))
    assert util.rel_err(ipred, out["ipred"].numpy()) < 1e-4
    _assert_grads(g_hip, grads, prob, name)


def test_dynamic_lds_mark_is_kept_per_kernel_instance():
    """The launch helper (csrc/cl_kernels.h: cl_launch_lds) remembers, per kernel INSTANCE, the largest dynamic-LDS size it has
    configured.  In one process and in this order: the LDS-row lane instance of width 10 at its smallest need (16 metadata columns),
    the same instance at its largest (31 columns: the mark has to rise), then another instance of the same function-pointer type
    (width 4 on 31 columns: it has to be configured on its own account).  A mark that did not rise, or one shared between instances,
    shows as a launch error code; each step is held to the oracle like every other lane shape."""
    for w, d in ((10, 16), (10, 31), (4, 31)):
        out, grads, ipred, terms, g_hip, eng, prob = _run_case(dict(N=256, R=32, d0=d, L=20, w=w, S=1, perturb=0.02))
        # (the run above injects noise: the FULL form of the instance the production step is named after)
        assert eng.d == d and eng.kernel_name().startswith(f"elbo_lane_kernel<{w}, 0, false, "), (eng.d, eng.kernel_name())
        _assert_grads(g_hip, grads, prob, f"lds_mark_20x{w}_d{d}")


def _random_engine_cases(n=12, seed=11):
    """Seeded random draws over everything the engine routes: widths 1 .. 100 (lane / narrow / 32- and 64-wide fused instances,
    chains of launches for deep scalers, the own GEMM kernels of csrc/wide_gemm.hip beyond width 64), depths 1 .. 24, 1 .. 40 metadata columns, 1 .. 12 MC samples,
    mono / Laue / double-Wilson / per-image layers, every likelihood, bijector and reduction switch."""
    rng = np.random.default_rng(seed)
    cases = {}
    for i in range(n):
        kind = ["mono", "mono", "mono", "laue", "double_wilson", "image_layers"][int(rng.integers(0, 6))]
        w = int(rng.choice([rng.integers(1, 16), rng.integers(16, 33), rng.integers(33, 65), rng.integers(65, 101)], p=[0.4, 0.25, 0.25, 0.1]))
        L = int(rng.choice([rng.integers(1, 6), rng.integers(6, 21), rng.integers(21, 25)], p=[0.5, 0.4, 0.1]))
        S = int(rng.integers(1, 13))
        kw = dict(N=int(rng.integers(3, 1200)), R=int(rng.integers(2, 70)), L=L, w=w, S=S, perturb=0.02 if L > 8 else 0.05)
        if kind == "laue":
            kw["laue"] = True
            kw["N"] = max(kw["N"], 100)
            if rng.random() < 0.3:
                kw["two_pass"] = True
        else:
            kw["d0"] = int(rng.integers(1, 41)) if rng.random() < 0.7 else 5
            if kind == "mono" and rng.random() < 0.2:
                kw["posenc"] = True
                kw["d0"] = 5
        if kind == "double_wilson":
            kw["double_wilson"] = True
            kw["R"] = max(kw["R"], 8)
            if rng.random() < 0.4:
                kw["optimize_dw_r"] = True
        if kind == "image_layers":
            kw["image_layers"] = int(rng.integers(1, 3))
            kw["n_images"] = int(rng.integers(2, 8))
            kw["w"] = min(kw["w"], 64)
            kw["L"] = min(kw["L"], 10)
            kw["N"] = max(kw["N"], 50)
        elif rng.random() < 0.3 and kind == "mono":
            kw["shuffle_rows"] = True
            kw["n_images"] = int(rng.integers(2, 12))
        if rng.random() < 0.5:
            kw.update(likelihood="studentt", dof=float(rng.choice([3.0, 8.0, 32.0])))
        if rng.random() < 0.25 and kind != "double_wilson":
            kw["ev11"] = True
        if rng.random() < 0.3:
            kw.update(bijector="softplus", shift=float(rng.choice([0.0, 1.5])))
        if rng.random() < 0.25:
            kw["kl_weight"] = 0.5
        if rng.random() < 0.25 and kind != "image_layers":
            kw["use_image_scales"] = False
        if rng.random() < 0.4:
            kw["grid"] = int(rng.integers(1, 4))
        kw["R"] = min(kw["R"], kw["N"])
        one_launch = 20 if kw["w"] <= 15 else (10 if kw["w"] <= 32 else 5)         # layers one fused launch holds at this width
        if kind == "image_layers":
            # Dense + per-image layers must fit one launch (deeper ones raise NotImplementedError: DESIGN.md 4.7)
            kw["L"] = max(1, min(kw["L"], (16 if kw["w"] <= 15 else one_launch) - kw["image_layers"]))
        if kind == "laue" and kw["w"] <= 64:
            kw["L"] = min(kw["L"], one_launch)     # (chained scalers take the two-pass Laue path; _run_case asserts the single pass)
        if kind == "double_wilson":
            kw["R"] += kw["R"] % 2                 # two half-datasets of R / 2 reflections
            kw["N"] = max(kw["N"], kw["R"])
        if kw.get("n_images") == 1:
            kw["use_image_scales"] = False
        cases[f"random_{i:02d}_{kind}_{kw['L']}x{kw['w']}_S{S}"] = kw
    return cases


def _random_lane_image_layer_cases(n=10, seed=23, depths=False):
    """Seeded random draws over what the lane kernel's per-image-layer instances take (round 5: 20 Dense layers, width 1 .. 10, 1 .. 15 metadata
    columns, one or two per-image layers, mono and single-pass Laue, any sample count, every likelihood / bijector / reduction switch)."""
    rng = np.random.default_rng(seed)
    cases = {}
    for i in range(n):
        laue = rng.random() < 0.3
        kw = dict(N=int(rng.integers(60, 2500)), R=int(rng.integers(4, 90)), L=20, w=int(rng.integers(1, 11)), S=int(rng.integers(1, 13)),
                  image_layers=int(rng.integers(1, 3)), n_images=int(rng.integers(2, 30)), perturb=0.03)
        if depths:                      # (round 6: 2 .. 19 Dense layers at widths 5 .. 10, more than 15 columns behind a peeled first layer)
            kw.update(L=int(rng.integers(2, 20)), w=int(rng.integers(5, 11)))
        if rng.random() < 0.3:
            kw["image_layers"] = 3      # (round 6: a third per-image layer)
        if laue:
            kw["laue"] = True
            kw["N"] = max(kw["N"], 150)
            kw["n_images"] = min(kw["n_images"], 8)
        else:
            kw["d0"] = int(rng.integers(1, 16)) if not depths or rng.random() < 0.7 else int(rng.integers(16, 41))
            if rng.random() < 0.3:
                kw["shuffle_rows"] = True
        if rng.random() < 0.5:
            kw.update(likelihood="studentt", dof=float(rng.choice([3.0, 8.0, 32.0])))
        if rng.random() < 0.3:
            kw["ev11"] = True
        if rng.random() < 0.3:
            kw.update(bijector="softplus", shift=float(rng.choice([0.0, 1.5])))
        if rng.random() < 0.25:
            kw["kl_weight"] = 0.5
        if rng.random() < 0.4:
            kw["grid"] = int(rng.integers(1, 4))
        kw["R"] = min(kw["R"], kw["N"])
        cases[f"random_lane_imgl_{'depth_' if depths else ''}{i:02d}_{'laue' if laue else 'mono'}_{kw['L']}x{kw['w']}_K{kw['image_layers']}_S{kw['S']}"] = kw
    return cases


def _random_lane_depth_cases(n=16, seed=61):
    """Seeded random draws over round 6's routes around the default scaler: widths 5 .. 12 at any depth 2 .. 40 (the lane kernel compiled per
    depth, chains of lane blocks past 20 layers), 1 .. 40 metadata columns (past 15: the peeled first layer in front of the depth's dZ_0-storing
    instance), mono / single-pass Laue / double-Wilson, any sample count, every likelihood / bijector / reduction switch."""
    rng = np.random.default_rng(seed)
    cases = {}
    for i in range(n):
        kind = str(rng.choice(["mono", "laue", "double_wilson"], p=[0.6, 0.25, 0.15]))
        L = int(rng.choice([rng.integers(2, 20), rng.integers(21, 41)], p=[0.75, 0.25]))
        kw = dict(N=int(rng.integers(40, 1500)), R=int(rng.integers(4, 70)), L=L, w=int(rng.integers(5, 13)), S=int(rng.integers(1, 13)),
                  perturb=0.02 if L > 8 else 0.04)
        if L > 20:
            kw["perturb"] = 0.01
        if kind == "laue":
            kw["laue"] = True
            kw["L"] = min(kw["L"], 20)
            kw["N"] = max(kw["N"], 150)
            if rng.random() < 0.4:
                kw["extra_meta"] = int(rng.integers(1, 9))
        else:
            kw["d0"] = int(rng.integers(1, 41)) if rng.random() < 0.6 else 5
        if kind == "double_wilson":
            kw["double_wilson"] = True
            kw["R"] = max(kw["R"], 8)
            kw["R"] += kw["R"] % 2
            kw["N"] = max(kw["N"], kw["R"])
        if rng.random() < 0.5:
            kw.update(likelihood="studentt", dof=float(rng.choice([3.0, 8.0, 32.0])))
        if rng.random() < 0.25 and kind != "double_wilson":
            kw["ev11"] = True
        if rng.random() < 0.3:
            kw.update(bijector="softplus", shift=float(rng.choice([0.0, 1.5])))
        if rng.random() < 0.25:
            kw["kl_weight"] = 0.5
        if rng.random() < 0.25:
            kw["use_image_scales"] = False
        if rng.random() < 0.4:
            kw["grid"] = int(rng.integers(1, 4))
        kw["R"] = min(kw["R"], kw["N"])
        cases[f"random_lane_depth_{i:02d}_{kind}_{kw['L']}x{kw['w']}_S{kw['S']}"] = kw
    return cases


# (a longer sweep on demand: ENGINE_RANDOM_N=150 ENGINE_RANDOM_SEED=3 python -m pytest tests/test_gpu_parity.py -k random_engine)
RANDOM_ENGINE_CASES = _random_engine_cases(int(os.environ.get("ENGINE_RANDOM_N", "12")), int(os.environ.get("ENGINE_RANDOM_SEED", "11")))
RANDOM_ENGINE_CASES.update(_random_lane_depth_cases(int(os.environ.get("LANE_DEPTH_RANDOM_N", "16")), int(os.environ.get("ENGINE_RANDOM_SEED", "11")) + 50))
RANDOM_ENGINE_CASES.update(_random_lane_image_layer_cases(int(os.environ.get("LANE_IMGL_RANDOM_N", "10")), int(os.environ.get("ENGINE_RANDOM_SEED", "11")) + 12))
RANDOM_ENGINE_CASES.update(_random_lane_image_layer_cases(int(os.environ.get("LANE_IMGL_DEPTH_RANDOM_N", "12")), int(os.environ.get("ENGINE_RANDOM_SEED", "11")) + 31, depths=True))


@pytest.mark.parametrize("name", list(RANDOM_ENGINE_CASES))
def test_random_engine_configurations(name):
    out, grads, ipred, terms, g_hip, eng, prob = _run_case(RANDOM_ENGINE_CASES[name])
    assert abs(terms["nll"] - float(out["nll"])) <= RTOL_LOSS * abs(float(out["nll"])), (terms, float(out["nll"]))
    assert abs(terms["kl"] - float(out["kl"])) <= RTOL_LOSS * max(abs(float(out["kl"])), 1.0), (terms, float(out["kl"]))
    assert util.rel_err(ipred, out["ipred"].numpy()) < 1e-4
    _assert_grads(g_hip, grads, prob, name)


def test_deterministic_mode_refuses_per_image_layers_off_the_lane_kernel():
    """the IMGL instances of elbo_mlp.hip keep their float atomics: the mode raises instead of running with them"""
    from careless_amd.engine import ElboEngine
    for kw in (dict(N=500, R=40, d0=5, L=2, w=32, S=2, n_images=5, image_layers=1), dict(N=500, R=40, d0=5, L=20, w=10, S=2, n_images=5, image_layers=4)):
        data, cfg, params, x, u_f, eta = util.make_problem(**kw)
        model = util.build_model(data, cfg, params, kw["L"], kw["w"])
        model.deterministic = True
        with pytest.raises(NotImplementedError):
            ElboEngine(model, util.reference_inputs(data), seed=1)


def test_refl_gather_is_bit_exact():
    """ipred = z_scale * z_f[refl_id]^2: with loc=1, sigma~0 and no image scales, ipred/1 must equal z_f[refl_id]^2 exactly."""
    kw = dict(N=300, R=40, d0=5, L=2, w=32, S=2, use_image_scales=False, perturb=0.0)
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    # make the scaler output exactly loc = 1, raw = -80 (sigma = eps): zero weights, bias (1, -80)
    for wt in params.mlp_w:
        wt.zero_()
    params.mlp_b[-1][0] = 1.0
    params.mlp_b[-1][1] = -80.0
    cfg.epsilon = 0.0
    model = util.build_model(data, cfg, params, 2, 32)
    model.surrogate_posterior.scale_shift = 1e-7
    ipred = model(util.reference_inputs(data), u_f=u_f, eta=np.zeros_like(eta)).cpu().numpy()
    eng = model._engine
    z_f = eng.z_f.view(eng.R, eng.S).t().cpu().numpy()            # (S, R)
    rid = np.asarray(data["refl_id"])
    expect = (z_f[:, rid].astype(np.float32) ** 2).astype(np.float32)
    assert np.array_equal(ipred, expect * np.float32(1.0))


@pytest.mark.parametrize("L,w,d0", [(2, 32, 5), (20, 10, 5), (2, 96, 5), (20, 10, 37)], ids=["2x32", "cli_default_20x10", "wide_2x96", "peel_20x10_d37"])
def test_adam_trajectory_matches_oracle(L, w, d0):
    """20 Adam steps on injected noise: history and final parameters follow the oracle; also for the CLI-default geometry, which
    runs on the narrow instance (permuted features, LDS-resident accumulators, bias gradient in column 15), and for that geometry on 37
    metadata columns (peeled first layer: its parameters are updated from cl_peel_backward's gradient)"""
    kw = dict(N=384, R=48, d0=d0, L=L, w=w, S=2)
    data, cfg, params, x, u_f0, eta0 = util.make_problem(**kw)
    steps = 20
    rng = np.random.default_rng(11)
    noises = [(rng.random((2, 48)).astype(np.float32), rng.normal(size=(2, 384)).astype(np.float32)) for _ in range(steps)]
    model = util.build_model(data, cfg, params, L, w)
    hist = model.train_model(util.reference_inputs(data), steps, progress=False, noise=lambda i: noises[i])
    p = params.clone()
    st = O.AdamState.zeros_like(p.tensors())
    ref = [O.train_step(p, x, cfg, st, torch.as_tensor(u, dtype=torch.float64), torch.as_tensor(e, dtype=torch.float64))
           for u, e in noises]
    for k in ("loss", "NLL", "F KLDiv", "Grad Norm"):
        a = np.array(hist[k]); b = np.array([r[k] for r in ref])
        assert np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)) < 2e-4, (k, a, b)
    q = model.surrogate_posterior
    assert util.rel_err(q.loc_raw.cpu().numpy(), p.q_loc_raw.numpy()) < 1e-4
    assert util.rel_err(q.scale_raw.cpu().numpy(), p.q_scale_raw.numpy()) < 1e-4
    eng = model._engine
    for a, b in zip(eng.mlp.weights, [t for pair in zip(p.mlp_w, p.mlp_b) for t in pair]):
        assert util.rel_err(a.cpu().numpy(), b.numpy()) < 2e-4


def test_trainable_double_wilson_r_trajectory():
    """--optimize-double-wilson-r: r = sigmoid(raw) follows the oracle's Adam trajectory and is logged as rDW_i
    (reference priors/wilson.py:105-110, 173-174)."""
    kw = dict(N=400, R=60, d0=5, L=2, w=32, S=4, double_wilson=True, optimize_dw_r=True)
    data, cfg, params, x, _, _ = util.make_problem(**kw)
    steps = 12
    rng = np.random.default_rng(5)
    noises = [(rng.random((4, 60)).astype(np.float32), rng.normal(size=(4, 400)).astype(np.float32)) for _ in range(steps)]
    model = util.build_model(data, cfg, params, 2, 32)
    hist = model.train_model(util.reference_inputs(data), steps, progress=False, noise=lambda i: noises[i])
    p = params.clone()
    st = O.AdamState.zeros_like(p.tensors())
    r_ref = []
    for u, e in noises:
        r_ref.append(torch.sigmoid(p.dw_r_raw).numpy().copy())
        O.train_step(p, x, cfg, st, torch.as_tensor(u, dtype=torch.float64), torch.as_tensor(e, dtype=torch.float64))
    r_ref = np.array(r_ref)
    assert np.all(np.array(hist["rDW_0"]) == 0.0)                       # the root ASU has no parent: r stays 0
    assert np.max(np.abs(np.array(hist["rDW_1"]) - r_ref[:, 1])) < 2e-5
    assert abs(r_ref[-1, 1] - r_ref[0, 1]) > 5e-4                        # it did move
    assert np.allclose(model.prior.r, torch.sigmoid(p.dw_r_raw).numpy(), atol=2e-5)


def test_philox_mode_matches_oracle_on_dumped_noise():
    """Production mode draws the noise in-kernel; dump the same stream with cl_debug_noise and replay it through the oracle."""
    from careless_amd.engine import debug_noise
    kw = dict(N=300, R=40, d0=5, L=2, w=32, S=3)
    data, cfg, params, x, _, _ = util.make_problem(**kw)
    model = util.build_model(data, cfg, params, 2, 32)
    model.seed = 4321
    ipred = model(util.reference_inputs(data))
    eng = model._engine
    torch.cuda.synchronize()
    u = debug_noise(4321, 0, 3, 40, 0, kind=0).t().cpu().numpy()      # (S, R)
    e = debug_noise(4321, 0, 3, 300, 0, kind=1).t().cpu().numpy()     # (S, N)
    assert 0.0 < u.min() and u.max() < 1.0
    out, grads = O.elbo_value_and_grads(params, x, cfg, torch.as_tensor(u, dtype=torch.float64),
                                        torch.as_tensor(e, dtype=torch.float64))
    t = eng.loss_terms()
    assert abs(t["loss"] - float(out["loss"])) <= 1e-4 * abs(float(out["loss"]))
    errs = [util.rel_err(a.cpu().numpy(), b.numpy()) for a, b in zip(eng.grad_tensors(), grads)]
    assert max(errs) < RTOL_GRAD, errs


def test_philox_mode_on_the_narrow_kernel_with_twelve_samples():
    """The narrow kernel walks the MC samples of an observation serially and shares one Box-Muller pair between samples s and
    s + 4 (cl_math.h: cl_noise_normal_pair): twelve samples go through every branch of that bookkeeping."""
    from careless_amd.engine import debug_noise
    kw = dict(N=333, R=40, d0=5, L=4, w=10, S=12, perturb=0.03)
    data, cfg, params, x, _, _ = util.make_problem(**kw)
    model = util.build_model(data, cfg, params, 4, 10)
    model.seed = 99
    model(util.reference_inputs(data))
    eng = model._engine
    torch.cuda.synchronize()
    u = debug_noise(99, 0, 12, 40, 0, kind=0).t().cpu().numpy()
    e = debug_noise(99, 0, 12, 333, 0, kind=1).t().cpu().numpy()
    out, grads = O.elbo_value_and_grads(params, x, cfg, torch.as_tensor(u, dtype=torch.float64), torch.as_tensor(e, dtype=torch.float64))
    t = eng.loss_terms()
    assert abs(t["loss"] - float(out["loss"])) <= 1e-4 * abs(float(out["loss"]))
    errs = [util.rel_err(a.cpu().numpy(), b.numpy()) for a, b in zip(eng.grad_tensors(), grads)]
    assert max(errs) < RTOL_GRAD, errs


@pytest.mark.parametrize("S,w,d0", [(8, 10, 5), (5, 6, 12), (1, 10, 5), (8, 10, 21), (13, 8, 27)],
                         ids=["S8_20x10", "S5_20x6_d12", "S1_20x10", "S8_20x10_d21", "S13_20x8_d27"])
def test_philox_mode_on_the_lane_kernel(S, w, d0):
    """The lane-per-observation kernel (20 layers) with in-kernel noise: every lane walks its observation's samples serially, samples
    s and s + 4 share a Box-Muller pair, the amplitudes of samples 1 .. 7 arrive through LDS and the amplitude gradients leave
    through it (csrc/elbo_lane.hip); 191 observations = two full wave tiles and a ragged third."""
    from careless_amd.engine import debug_noise
    kw = dict(N=191, R=40, d0=d0, L=20, w=w, S=S, perturb=0.02)
    data, cfg, params, x, _, _ = util.make_problem(**kw)
    model = util.build_model(data, cfg, params, 20, w)
    model.seed = 7
    model(util.reference_inputs(data))
    eng = model._engine
    torch.cuda.synchronize()
    u = debug_noise(7, 0, S, 40, 0, kind=0).t().cpu().numpy()
    e = debug_noise(7, 0, S, 191, 0, kind=1).t().cpu().numpy()
    out, grads = O.elbo_value_and_grads(params, x, cfg, torch.as_tensor(u, dtype=torch.float64), torch.as_tensor(e, dtype=torch.float64))
    t = eng.loss_terms()
    assert abs(t["loss"] - float(out["loss"])) <= 1e-4 * abs(float(out["loss"]))
    errs = [util.rel_err(a.cpu().numpy(), b.numpy()) for a, b in zip(eng.grad_tensors(), grads)]
    assert max(errs) < RTOL_GRAD, errs


@pytest.mark.parametrize("w,d0,posenc,S", [(10, 5, False, 1), (10, 5, True, 8), (6, 12, False, 3)], ids=["20x10_d5_S1", "20x10_d21_S8", "20x6_d12_S3"])
def test_lane_kernel_production_instance_equals_the_full_one(w, d0, posenc, S):
    """The lane kernel has two instances per shape: one with every optional input / output (injected noise, `ipred_out`, Ev11) --
    what the oracle-parity cases run -- and the one a production training step runs, without them.  Same in-kernel noise (same
    seed and step): the step that also returns its predictions (full instance) and the plain step must agree on every loss term
    and gradient to summation order."""
    from careless_amd.engine import ElboEngine
    kw = dict(N=2300, R=70, d0=d0, posenc=posenc, L=20, w=w, S=S, perturb=0.02, likelihood="studentt", dof=8.0, n_images=5)
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    inputs = util.reference_inputs(data)
    res = []
    for full in (False, True):
        eng = ElboEngine(util.build_model(data, cfg, params, 20, w), inputs, seed=11)
        ipred = torch.zeros(kw["N"] * S, dtype=torch.float32, device=eng.device) if full else None
        eng.forward_backward(3, ipred_out=ipred)
        torch.cuda.synchronize()
        name = eng.kernel_name()
        assert name.startswith("elbo_lane_kernel<") and name.endswith(", false, false>")      # (the name is asked for without ipred_out)
        res.append((eng.loss_terms(), eng.grads.clone(), ipred))
    (ta, ga, _), (tb, gb, ip) = res
    assert abs(ta["nll"] - tb["nll"]) <= 1e-7 * abs(tb["nll"]) and ta["kl"] == tb["kl"]
    assert util.rel_err(ga.cpu().numpy(), gb.cpu().numpy()) < 2e-5
    assert bool(torch.isfinite(ip).all()) and float(ip.abs().max()) > 0


@pytest.mark.parametrize("S,img,w,N", [(3, True, 128, 2117), (4, True, 128, 2117), (4, False, 128, 2117), (9, True, 128, 2117), (2, True, 100, 1301),
                                       (4, True, 128, 66000)],
                         ids=["S3_rows_straddle_waves", "S4_rows_inside_waves", "S4_no_image_scales", "S9_three_samples_a_lane", "w100_seven_blocks",
                              "rows66000_waves_walk_two_blocks"])
def test_wide_fused_backward_equals_the_separate_launches(monkeypatch, S, img, w, N):
    """Round 4 folded three launches of the layer-by-layer path into their neighbours: the first layer's weight gradient into the second
    layer's dgrad, the Dense(2) head's backward pass into the top layer's weight gradient and dgrad, predict / log-prob / gradient of
    rows that are their own slot into one kernel (S = 3: a row's samples straddle waves -- dO by atomics; S = 4: stored) and that
    kernel into the top layer's forward epilogue.  The class switches bring the separate launches back; same in-kernel noise: every loss term and gradient must agree to summation order.
    w = 100: the seven-block instances (wide_sq_kernel<.., 7> with WG0 / HEADB / LIK); N = 66 000: more 16-row blocks than the 2 CUs x 8 waves of
    the grid, so the fused likelihood epilogue, HEADB and WG0 cross a block boundary inside a wave (they run on in-kernel noise only)."""
    from careless_amd.engine import ElboEngine
    kw = dict(N=N, R=90, d0=8, L=3, w=w, S=S, perturb=0.02, likelihood="studentt", dof=10.0, n_images=5, use_image_scales=img)
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    inputs = util.reference_inputs(data)
    res = []
    for fused in (True, False):
        for k in ("FUSE_WG0", "FUSE_HEADB", "FUSE_LIK", "SLOT_ROWS_ONE_LAUNCH"):
            monkeypatch.setattr(ElboEngine, k, fused)
        eng = ElboEngine(util.build_model(data, cfg, params, 3, w), inputs, seed=5)
        assert eng.wide
        eng.forward_backward(2)
        torch.cuda.synchronize()
        res.append((eng.loss_terms(), eng.grads.clone()))
    (ta, ga), (tb, gb) = res
    # The NLL is an fp64 sum over rows of fp32 per-row terms on both sides; the two sides differ by the rounding of each row's term (the
    # fused epilogue takes (loc, sigma) from registers in another summation order: relative error e_row of a few u = 2^-24 per term, far
    # inside 5e-7) -- independent from row to row, so the sum's relative difference is at most e_row where the terms are of one sign and
    # shrinks like 1 / sqrt(N) otherwise: the limit does NOT grow with the row count and stays 5e-7 at every N.
    assert abs(ta["nll"] - tb["nll"]) <= 5e-7 * abs(tb["nll"]) and ta["kl"] == tb["kl"]     # (round 5: the fused epilogue sums rows in fp64 like the separate launch)
    assert util.rel_err(ga.cpu().numpy(), gb.cpu().numpy()) < 2e-5
    for a, b in zip(eng._split(ga), eng._split(gb)):           # tensor by tensor: the head, every layer, the image scales
        assert util.rel_err(a.cpu().numpy(), b.cpu().numpy()) < 5e-5


@pytest.mark.parametrize("keep", [True, False], ids=["activations_kept", "forward_recomputed_per_chunk"])
def test_wide_path_in_several_row_chunks_equals_one_chunk(monkeypatch, keep):
    """The layer-by-layer path walks the observations in row chunks sized from a memory budget, and keeps all activations only when they
    fit (otherwise every chunk's forward pass is run again when its turn in the backward pass comes).  With the budgets lowered to five
    chunks of 512 rows (and no kept activations): the gradient sums over the chunks, the head's dsigma/draw of the first pass feeds the
    fused backward kernels of the second -- the same step as with one chunk, to summation order."""
    from careless_amd.engine import ElboEngine
    from careless_amd.wide import WidePath
    kw = dict(N=2117, R=90, d0=8, L=3, w=128, S=2, perturb=0.02, likelihood="studentt", dof=10.0, n_images=5)
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    inputs = util.reference_inputs(data)
    eng = ElboEngine(util.build_model(data, cfg, params, 3, 128), inputs, seed=5)
    eng.forward_backward(2)
    torch.cuda.synchronize()
    assert len(eng._wide_chunks(eng.obs)) == 1
    ta, ga = eng.loss_terms(), eng.grads.clone()
    monkeypatch.setattr(WidePath, "WIDE_BUDGET", 4 * (3 + 2) * 128 * 600)          # 600 rows of the five row buffers: chunks of 512
    if not keep:
        monkeypatch.setattr(WidePath, "WIDE_KEEP_BUDGET", 0)
    eng2 = ElboEngine(util.build_model(data, cfg, params, 3, 128), inputs, seed=5)
    eng2.forward_backward(2)
    torch.cuda.synchronize()
    assert len(eng2._wide_chunks(eng2.obs)) == 5
    assert (getattr(eng2.obs, "wide_full", None) is not None) == keep
    tb, gb = eng2.loss_terms(), eng2.grads
    assert abs(ta["nll"] - tb["nll"]) <= 1e-6 * abs(ta["nll"]) and ta["kl"] == tb["kl"]
    for a, b in zip(eng._split(ga), eng2._split(gb)):
        assert util.rel_err(a.cpu().numpy(), b.cpu().numpy()) < 5e-5


def test_image_layers_philox_noise_is_keyed_by_the_callers_rows():
    """--image-layers packs the observations by image inside the engine; the in-kernel noise must still be keyed by the caller's
    row index (rows arrive in arbitrary image order here), so the dumped stream replayed through the oracle gives the same loss."""
    from careless_amd.engine import debug_noise
    kw = dict(N=500, R=40, d0=5, L=2, w=32, S=3, n_images=5, image_layers=1)
    data, cfg, params, x, _, _ = util.make_problem(**kw)
    perm = np.random.default_rng(3).permutation(kw["N"])
    for k in ("refl_id", "image_id", "file_id", "metadata", "iobs", "sigiobs"):
        data[k] = np.asarray(data[k])[perm]
    x = O.inputs_from_numpy(data)
    model = util.build_model(data, cfg, params, 2, 32)
    model.seed = 77
    ipred = model(util.reference_inputs(data)).cpu().numpy()
    eng = model._engine
    torch.cuda.synchronize()
    u = debug_noise(77, 0, 3, 40, 0, kind=0).t().cpu().numpy()
    e = debug_noise(77, 0, 3, 500, 0, kind=1).t().cpu().numpy()
    out, grads = O.elbo_value_and_grads(params, x, cfg, torch.as_tensor(u, dtype=torch.float64), torch.as_tensor(e, dtype=torch.float64))
    t = eng.loss_terms()
    assert abs(t["loss"] - float(out["loss"])) <= 1e-4 * abs(float(out["loss"]))
    assert util.rel_err(ipred, out["ipred"].numpy()) < 1e-4
    errs = [util.rel_err(a.cpu().numpy(), b.numpy()) for a, b in zip(eng.grad_tensors(), grads)]
    assert len(errs) == len(grads) and max(errs) < RTOL_GRAD, errs


@pytest.mark.parametrize("kw", [dict(N=2500, R=60, d0=5, L=20, w=10, S=2, n_images=13, image_layers=2, perturb=0.03),
                                dict(N=1800, R=50, d0=11, L=20, w=8, S=1, n_images=9, image_layers=1, likelihood="studentt", dof=8.0, perturb=0.03),
                                dict(N=2000, R=60, d0=5, posenc=True, L=20, w=10, S=2, n_images=9, image_layers=2, perturb=0.03)],
                         ids=["20x10_img2", "20x8_d11_img1_studentt", "20x10_img2_posenc_d21_peeled"])
def test_lane_image_layers_production_instance_on_in_kernel_noise(kw):
    """`--image-layers` on the default scaler, as a production step runs it (round 5: elbo_lane_kernel<.., NI> without the optional
    inputs / outputs, in-kernel Philox noise keyed by the caller's rows through the by-image packing): the dumped noise replayed through
    the oracle gives the same loss and gradients, per-image tensors included."""
    from careless_amd.engine import ElboEngine, debug_noise
    data, cfg, params, x, _, _ = util.make_problem(**kw)
    perm = np.random.default_rng(3).permutation(kw["N"])
    for k in ("refl_id", "image_id", "file_id", "metadata", "iobs", "sigiobs"):
        data[k] = np.asarray(data[k])[perm]
    x = O.inputs_from_numpy(data)
    eng = ElboEngine(util.build_model(data, cfg, params, kw["L"], kw["w"]), util.reference_inputs(data), seed=77)
    eng.forward_backward(5)
    torch.cuda.synchronize()
    name = eng.kernel_name()
    peeled = np.asarray(data["metadata"]).shape[1] > 15          # (behind a peeled first layer the production instance that stores dZ_0 runs: back in round 6)
    assert name.startswith("elbo_lane_kernel<10, ") and f"true, false, {'true' if peeled else 'false'}, {kw['image_layers']}>" in name, name
    u = debug_noise(77, 5, kw["S"], kw["R"], 0, kind=0).t().cpu().numpy()
    e = debug_noise(77, 5, kw["S"], kw["N"], 0, kind=1).t().cpu().numpy()
    out, grads = O.elbo_value_and_grads(params, x, cfg, torch.as_tensor(u, dtype=torch.float64), torch.as_tensor(e, dtype=torch.float64))
    t = eng.loss_terms()
    assert abs(t["loss"] - float(out["loss"])) <= RTOL_LOSS * abs(float(out["loss"]))
    _assert_grads([g.cpu().numpy() for g in eng.grad_tensors()], grads, (data, cfg, params, u, e), name="lane image layers, in-kernel noise")


# (test_lane_production_instances_repeat_from_run_to_run, round 5's guard over ten lane instances, became tests/test_lane_repeat.py in
#  round 6: every instance, bit-identical scaler gradients, 5 000 and 4 M rows.)


def test_image_layers_adam_trajectory_and_scaler_call():
    kw = dict(N=600, R=48, d0=5, L=2, w=16, S=2, n_images=4, image_layers=2)
    data, cfg, params, x, _, _ = util.make_problem(**kw)
    steps = 10
    rng = np.random.default_rng(11)
    noises = [(rng.random((2, 48)).astype(np.float32), rng.normal(size=(2, 600)).astype(np.float32)) for _ in range(steps)]
    model = util.build_model(data, cfg, params, 2, 16)
    inputs = util.reference_inputs(data)
    # scaler(inputs) before training: NeuralImageScaler.call (image.py:116-125)
    dist = model.scaling_model(inputs)
    o = O.mlp_forward(x.metadata, params.mlp_w, params.mlp_b, cfg.leakiness, x.image_id, params.imgl_w, params.imgl_b)
    assert util.rel_err(dist.loc.cpu().numpy(), o[:, 0].numpy()) < 1e-5
    assert util.rel_err(dist.scale.cpu().numpy(), O.scale_bijector(o[:, 1], "exp", cfg.epsilon).numpy()) < 1e-5
    hist = model.train_model(inputs, steps, progress=False, noise=lambda i: noises[i])
    p = params.clone()
    st = O.AdamState.zeros_like(p.tensors())
    ref = [O.train_step(p, x, cfg, st, torch.as_tensor(u, dtype=torch.float64), torch.as_tensor(e, dtype=torch.float64))
           for u, e in noises]
    for k in ("loss", "NLL", "F KLDiv", "Grad Norm"):
        a = np.array(hist[k]); b = np.array([r[k] for r in ref])
        assert np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)) < 2e-4, (k, a, b)
    for a, b in zip(model.scaling_model.image_weights, [t for pair in zip(p.imgl_w, p.imgl_b) for t in pair]):
        assert util.rel_err(a.cpu().numpy(), b.numpy()) < 2e-4
    # predictions through the trained model (prediction_mean_stddev -> scaler forward with image layers)
    mean, std = model.scale_mean_stddev(inputs)
    o = O.mlp_forward(x.metadata, p.mlp_w, p.mlp_b, cfg.leakiness, x.image_id, p.imgl_w, p.imgl_b)
    assert util.rel_err(_np(mean).reshape(-1), o[:, 0].detach().numpy()) < 2e-4


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def test_wide_image_layers_adam_trajectory_and_scaler_call():
    """--image-layers on a scaler wider than 64 (layer-by-layer path, grouped per-image GEMMs): `scaler(inputs)`, an 8-step Adam
    trajectory and the prediction path against the oracle; rows arrive in arbitrary image order."""
    kw = dict(N=500, R=40, d0=5, L=2, w=72, S=2, n_images=5, image_layers=2)
    data, cfg, params, x, _, _ = util.make_problem(**kw)
    perm = np.random.default_rng(3).permutation(kw["N"])
    for k in ("refl_id", "image_id", "file_id", "metadata", "iobs", "sigiobs"):
        data[k] = np.asarray(data[k])[perm]
    x = O.inputs_from_numpy(data)
    steps = 8
    rng = np.random.default_rng(11)
    noises = [(rng.random((2, 40)).astype(np.float32), rng.normal(size=(2, 500)).astype(np.float32)) for _ in range(steps)]
    model = util.build_model(data, cfg, params, 2, 72)
    inputs = util.reference_inputs(data)
    dist = model.scaling_model(inputs)
    o = O.mlp_forward(x.metadata, params.mlp_w, params.mlp_b, cfg.leakiness, x.image_id, params.imgl_w, params.imgl_b)
    assert util.rel_err(dist.loc.cpu().numpy(), o[:, 0].numpy()) < 1e-5
    assert util.rel_err(dist.scale.cpu().numpy(), O.scale_bijector(o[:, 1], "exp", cfg.epsilon).numpy()) < 1e-5
    hist = model.train_model(inputs, steps, progress=False, noise=lambda i: noises[i])
    assert model._engine.wide and model._engine.imgl is not None
    p = params.clone()
    st = O.AdamState.zeros_like(p.tensors())
    ref = [O.train_step(p, x, cfg, st, torch.as_tensor(u, dtype=torch.float64), torch.as_tensor(e, dtype=torch.float64))
           for u, e in noises]
    for k in ("loss", "NLL", "F KLDiv", "Grad Norm"):
        a = np.array(hist[k]); b = np.array([r[k] for r in ref])
        assert np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)) < 2e-4, (k, a, b)
    for a, b in zip(model.scaling_model.image_weights, [t for pair in zip(p.imgl_w, p.imgl_b) for t in pair]):
        assert util.rel_err(a.cpu().numpy(), b.numpy()) < 2e-4
    mean, std = model.scale_mean_stddev(inputs)
    o = O.mlp_forward(x.metadata, p.mlp_w, p.mlp_b, cfg.leakiness, x.image_id, p.imgl_w, p.imgl_b)
    assert util.rel_err(_np(mean).reshape(-1), o[:, 0].detach().numpy()) < 2e-4


def test_chained_deep_scaler_trajectory_validation_and_predictions():
    """13 layers of width 32 = two launches per pass (10 is the most one launch holds): Adam trajectory against the oracle,
    NLL_val, and the prediction path (`scaler(inputs)` chains its forward the same way)."""
    kw = dict(N=500, R=40, d0=5, L=13, w=32, S=2)
    data, cfg, params, x, _, _ = util.make_problem(**kw)
    steps = 8
    rng = np.random.default_rng(3)
    noises = [(rng.random((2, 40)).astype(np.float32), rng.normal(size=(2, 500)).astype(np.float32)) for _ in range(steps)]
    model = util.build_model(data, cfg, params, 13, 32)
    inputs = util.reference_inputs(data)
    hist = model.train_model(inputs, steps, progress=False, noise=lambda i: noises[i])
    assert len(model._engine.blocks) == 2 and [b.l1 - b.l0 for b in model._engine.blocks] == [7, 6]
    p = params.clone()
    st = O.AdamState.zeros_like(p.tensors())
    ref = [O.train_step(p, x, cfg, st, torch.as_tensor(u, dtype=torch.float64), torch.as_tensor(e, dtype=torch.float64))
           for u, e in noises]
    for k in ("loss", "NLL", "F KLDiv", "Grad Norm"):
        a = np.array(hist[k]); b = np.array([r[k] for r in ref])
        assert np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)) < 2e-4, (k, a, b)
    mean, std = model.scale_mean_stddev(inputs)
    o = O.mlp_forward(x.metadata, p.mlp_w, p.mlp_b, cfg.leakiness)
    a_img = O.image_scales(p.img_raw)[x.image_id]
    assert util.rel_err(_np(mean).reshape(-1), (a_img * o[:, 0]).detach().numpy()) < 2e-4
    model2 = util.build_model(data, cfg, params, 13, 32)
    tr, te = tuple(a[:400] for a in inputs), tuple(a[400:] for a in inputs)
    h2 = model2.train_model(tr, 4, progress=False, validation_data=te, validation_frequency=2)
    assert len(h2["NLL_val"]) == 4 and all(np.isfinite(h2["NLL_val"]))


def test_noise_statistics_and_shard_independence():
    from careless_amd.engine import debug_noise
    e = debug_noise(1, 5, 4, 200000, 0, kind=1).cpu().numpy()
    assert abs(e.mean()) < 5e-3 and abs(e.std() - 1.0) < 5e-3
    u = debug_noise(1, 5, 4, 200000, 0, kind=0).cpu().numpy()
    assert abs(u.mean() - 0.5) < 3e-3 and abs(u.var() - 1.0 / 12.0) < 2e-3
    # keyed by the GLOBAL index: a shard starting at 1000 sees the same numbers
    part = debug_noise(1, 5, 4, 500, 1000, kind=1).cpu().numpy()
    assert np.array_equal(part, e[1000:1500])
    assert not np.array_equal(debug_noise(1, 6, 4, 500, 0, kind=1).cpu().numpy(), e[:500])


def test_scaler_forward_and_tn_sample():
    kw = dict(N=300, R=40, d0=5, L=5, w=64, S=1)
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    model = util.build_model(data, cfg, params, 5, 64)
    dist = model.scaling_model.mlp_scaler(util.reference_inputs(data))
    o = O.mlp_forward(x.metadata, params.mlp_w, params.mlp_b, cfg.leakiness)
    assert util.rel_err(dist.loc.cpu().numpy(), o[:, 0].numpy()) < 1e-5
    assert util.rel_err(dist.scale.cpu().numpy(), O.scale_bijector(o[:, 1], "exp", cfg.epsilon).numpy()) < 1e-5
    from careless_amd.engine import tn_sample
    z = tn_sample(model.surrogate_posterior, 1, u_f=u_f).cpu().numpy()
    loc, scale = O.tn_loc_scale(params.q_loc_raw, params.q_scale_raw, cfg.epsilon)
    zo = O.tn_sample(loc, scale, x.low, torch.tensor(cfg.high, dtype=torch.float64), torch.as_tensor(u_f, dtype=torch.float64))
    assert util.rel_err(z, zo.numpy()) < 1e-5


# --- the committed golden vectors (tests/golden/*.npz) through the HIP engine ------------------------------------------
from tests.test_golden import FILES as GOLDEN_FILES, load_case as load_golden  # noqa: E402
import os  # noqa: E402


@pytest.mark.parametrize("path", GOLDEN_FILES, ids=[os.path.basename(f) for f in GOLDEN_FILES])
def test_hip_engine_reproduces_golden_vectors(path):
    z, kw, data, cfg, params = load_golden(path)
    model = util.build_model(data, cfg, params, kw["L"], kw["w"])
    inputs = util.reference_inputs(data)
    ipred = model(inputs, u_f=z["u_f"], eta=z["eta"]).cpu().numpy()
    eng = model._engine
    t = eng.loss_terms()
    assert abs(t["loss"] - float(z["loss"])) <= RTOL_LOSS * abs(float(z["loss"]))
    assert abs(t["nll"] - float(z["nll"])) <= RTOL_LOSS * abs(float(z["nll"]))
    assert abs(t["kl"] - float(z["kl"])) <= RTOL_LOSS * max(abs(float(z["kl"])), 1.0)
    assert util.rel_err(ipred, z["ipred"]) < 1e-4
    errs = [util.rel_err(g.cpu().numpy(), z[f"grad_{i:02d}"]) for i, g in enumerate(eng.grad_tensors())]
    assert max(errs) < RTOL_GRAD, errs
    from tests.golden.make_golden import STEPS
    model2 = util.build_model(data, cfg, params, kw["L"], kw["w"])
    hist = model2.train_model(inputs, STEPS, progress=False, noise=lambda i: (z["traj_u"][i], z["traj_eta"][i]))
    assert np.max(np.abs(np.array(hist["loss"]) - z["traj_loss"]) / np.abs(z["traj_loss"])) < RTOL_LOSS
    assert np.max(np.abs(np.array(hist["Grad Norm"]) - z["traj_gnorm"]) / np.abs(z["traj_gnorm"])) < 2e-4
    finals = model2._engine.param_tensors()
    assert len(finals) == len([k for k in z.files if k.startswith("final_")])
    for i, tns in enumerate(finals):
        got, want = tns.cpu().numpy(), z[f"final_{i:02d}"]
        fin = np.isfinite(want)                  # logit(r = 0) = -inf for the root ASU of a double-Wilson model
        assert np.array_equal(got[~fin], want[~fin].astype(got.dtype)) and util.rel_err(got[fin], want[fin]) < 2e-4, i


def test_full_size_properties_1M():
    """BASELINE configs[1] at full size (1 M observations): properties that need no oracle -- determinism of the
    deterministic parts, linearity of the gradient in the loss weight, finite loss, loss decreases over a few steps."""
    from careless_amd.workloads import make_workload
    model, inputs, data, spec = make_workload("mono_1M_normal_5x64_S1")
    eng = model.engine(inputs)
    eng.forward_backward(0)
    torch.cuda.synchronize()
    a = eng.loss_terms()
    g1 = eng.grads.clone()
    kl1 = a["kl"]
    eng.forward_backward(0)
    torch.cuda.synchronize()
    b = eng.loss_terms()
    assert b["kl"] == kl1                                     # the KL path has no atomics: bitwise repeatable
    assert abs(a["nll"] - b["nll"]) <= 1e-9 * abs(a["nll"])   # NLL partials are summed in fp64
    assert torch.allclose(eng.grads, g1, rtol=1e-3, atol=1e-3 * float(g1.abs().max()))  # float-atomic order only
    # same noise key, different S-independent check: every reflection observed -> dz_f has no exact zeros in observed slots
    assert bool(torch.isfinite(eng.grads).all()) and float(eng.grads.abs().max()) > 0
    hist = model.train_model(inputs, 5, progress=False)
    assert len(hist["loss"]) == 5 and all(np.isfinite(hist["loss"])) and hist["loss"][-1] < hist["loss"][0]
    # ... and in deterministic mode (no atomics: stores + fixed-order sums) nothing differs at all, and it agrees with the default mode
    from careless_amd.engine import ElboEngine
    model2, inputs2, _, _ = make_workload("mono_1M_normal_5x64_S1")
    model2.deterministic = True
    det = [ElboEngine(model2, inputs2, seed=model.seed) for _ in range(2)]
    for e in det:
        e.forward_backward(0)
    torch.cuda.synchronize()
    assert torch.equal(det[0].grads, det[1].grads) and det[0].loss_terms() == det[1].loss_terms()
    assert torch.allclose(det[0].grads, g1, rtol=1e-3, atol=1e-3 * float(g1.abs().max()))


def _segments_close(lay, got, want, rtol=2e-4):
    for lo, hi in zip(lay.seg_off[:-1], lay.seg_off[1:]):                      # per trainable tensor (fp32 atomics: summation order only)
        a, b = got[lo:hi], want[lo:hi]
        assert float((a - b).abs().max()) <= rtol * max(float(b.abs().max()), 1e-6), (lo, hi)


def test_full_size_configs2_properties_10M(monkeypatch):
    """BASELINE configs[2] -- the configuration the headline metric is quoted on -- at FULL size (10 M observations x 21 metadata
    columns x 8 MC samples, Student-T, 5 x 64), in-kernel noise; properties that need no oracle and do not depend on the size:
    (a) the eight row shards of an 8-GPU job, run one after the other on this GPU without the all-reduce, add up to the single-GPU
    step; (b) the step cut into several launches (the 4-GiB bound lowered to a third of the metadata image) equals the single launch;
    (c) two deterministic-mode engines give bit-identical gradients and loss terms, and agree with the default mode."""
    from careless_amd.engine import ElboEngine, ObsChunks, make_shard
    from careless_amd.workloads import make_workload
    model, inputs, data, spec = make_workload("mono_10M_studentt_posenc_5x64_S8")
    assert spec["N"] == 10_000_000 and spec["d"] == 21 and spec["S"] == 8
    n, r = spec["N"], spec["R"]
    model.owner_shard = False
    full = ElboEngine(model, inputs, seed=7)
    assert not isinstance(full.obs, ObsChunks)
    full.forward_backward(1)
    torch.cuda.synchronize()
    g_full, t_full, lay = full.grads.clone(), full.loss_terms(), full.layout
    assert np.isfinite(t_full["loss"]) and bool(torch.isfinite(g_full).all())
    del full
    # (a) eight row shards
    g_sum, nll, kl = torch.zeros_like(g_full), 0.0, 0.0
    for rank in range(8):
        eng = ElboEngine(model, inputs, seed=7, shard=make_shard(n, r, rank, 8))
        assert not eng.owner and eng.N == n // 8
        eng.local_only = True
        eng.forward_backward(1)
        torch.cuda.synchronize()
        g_sum += eng.grads
        t = eng.loss_terms()
        nll += t["nll"]; kl += t["kl"]
        del eng
    assert abs(nll - t_full["nll"]) <= 1e-6 * abs(t_full["nll"]) and abs(kl - t_full["kl"]) <= 1e-6 * max(abs(t_full["kl"]), 1.0)
    _segments_close(lay, g_sum, g_full)
    # (b) cut into launches
    monkeypatch.setenv("CARELESS_HIP_MAX_LAUNCH_BYTES", str(4 * 24 * (n // 3 + 4096)))
    cut = ElboEngine(model, inputs, seed=7)
    monkeypatch.delenv("CARELESS_HIP_MAX_LAUNCH_BYTES")
    assert isinstance(cut.obs, ObsChunks) and len(cut.obs.children) == 3 and sum(c.N for c in cut.obs.children) == n
    cut.forward_backward(1)
    torch.cuda.synchronize()
    tc = cut.loss_terms()
    assert abs(tc["nll"] - t_full["nll"]) <= 1e-6 * abs(t_full["nll"]) and tc["kl"] == t_full["kl"]
    _segments_close(lay, cut.grads, g_full)
    del cut
    # (c) deterministic mode, twice
    model.deterministic = True
    runs = []
    for _ in range(2):
        e = ElboEngine(model, inputs, seed=7)
        assert e.deterministic
        e.forward_backward(1)
        torch.cuda.synchronize()
        runs.append((e.grads.clone(), e.loss_terms()))
        del e
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert abs(runs[0][1]["nll"] - t_full["nll"]) <= 1e-6 * abs(t_full["nll"])
    _segments_close(lay, runs[0][0], g_full)


def test_full_size_double_wilson_two_shards_sum_to_the_full_batch_10M():
    """BASELINE configs[4] (two-ASU double-Wilson prior, Normal likelihood, 5 x 64) at 10 M observations: the two row shards of a
    2-rank job add up to the single-GPU step (the parent scatter of the prior's gradient, the KL owned once, row-keyed noise)."""
    from careless_amd.engine import ElboEngine, make_shard
    from careless_amd.workloads import make_workload
    model, inputs, data, spec = make_workload("dw_50M_normal_5x64_S1", N=10_000_000)
    n, r = spec["N"], spec["R"]
    full = ElboEngine(model, inputs, seed=3)
    assert full.double_wilson
    full.forward_backward(2)
    torch.cuda.synchronize()
    g_full, t_full, lay = full.grads.clone(), full.loss_terms(), full.layout
    del full
    g_sum, nll, kl = torch.zeros_like(g_full), 0.0, 0.0
    for rank in range(2):
        eng = ElboEngine(model, inputs, seed=3, shard=make_shard(n, r, rank, 2))
        eng.local_only = True
        eng.forward_backward(2)
        torch.cuda.synchronize()
        g_sum += eng.grads
        t = eng.loss_terms()
        nll += t["nll"]; kl += t["kl"]
        del eng
    assert abs(nll - t_full["nll"]) <= 1e-6 * abs(t_full["nll"]) and abs(kl - t_full["kl"]) <= 1e-6 * max(abs(t_full["kl"]), 1.0)
    _segments_close(lay, g_sum, g_full)


def test_full_size_laue_single_pass_equals_two_pass():
    """BASELINE configs[3] shape at 1 M rows: the two Laue implementations (group sums as lane reductions inside the fused kernel
    vs. forward / group-sum / backward passes) draw the same in-kernel noise (keyed by the caller's rows) and must agree on the
    loss and on every gradient -- a size-independent check that needs no oracle."""
    from careless_amd.workloads import make_workload
    from careless_amd.engine import ElboEngine
    res = []
    for two_pass in (False, True):
        model, inputs, data, spec = make_workload("laue_5M_normal_5x64_S1", N=1_000_000)
        model.laue_two_pass = two_pass
        eng = ElboEngine(model, inputs, seed=5)
        assert eng.obs.fused_laue == (not two_pass)
        eng.forward_backward(2)
        torch.cuda.synchronize()
        res.append((eng.loss_terms(), eng.grads.clone()))
    (ta, ga), (tb, gb) = res
    assert abs(ta["nll"] - tb["nll"]) <= 1e-6 * abs(tb["nll"]) and ta["kl"] == tb["kl"]
    lay = eng.layout
    for lo, hi in zip(lay.seg_off[:-1], lay.seg_off[1:]):                      # per trainable tensor
        a, b = ga[lo:hi], gb[lo:hi]
        assert float((a - b).abs().max()) <= 2e-4 * max(float(b.abs().max()), 1e-6), (lo, hi)


@pytest.mark.parametrize("clip", [dict(clipnorm=0.5), dict(clipvalue=0.01), dict(global_clipnorm=1.0), dict(clipnorm=0.5, clipvalue=0.01),
                                  dict(global_clipnorm=1.0, clipvalue=0.01)])
def test_clipping_modes_match_oracle(clip):
    """tfk.optimizers.Adam(clipnorm= / clipvalue= / global_clipnorm=) (reference io/manager.py:494-501, tests/test_cli.py:196-208)"""
    kw = dict(N=300, R=40, d0=5, L=2, w=32, S=2, **clip)
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    steps = 4
    rng = np.random.default_rng(5)
    noises = [(rng.random((2, 40)).astype(np.float32), rng.normal(size=(2, 300)).astype(np.float32)) for _ in range(steps)]
    model = util.build_model(data, cfg, params, 2, 32)
    hist = model.train_model(util.reference_inputs(data), steps, progress=False, noise=lambda i: noises[i])
    p = params.clone()
    st = O.AdamState.zeros_like(p.tensors())
    ref = [O.train_step(p, x, cfg, st, torch.as_tensor(u, dtype=torch.float64), torch.as_tensor(e, dtype=torch.float64))
           for u, e in noises]
    assert np.allclose(hist["loss"], [r["loss"] for r in ref], rtol=1e-4)
    assert np.allclose(hist["Grad Norm"], [r["Grad Norm"] for r in ref], rtol=2e-4)
    assert util.rel_err(model.surrogate_posterior.loc_raw.cpu().numpy(), p.q_loc_raw.numpy()) < 1e-4
    for a, b in zip(model._engine.mlp.weights, [t for pair in zip(p.mlp_w, p.mlp_b) for t in pair]):
        assert util.rel_err(a.cpu().numpy(), b.numpy()) < 2e-4


def test_freeze_flags_and_early_stop():
    """--freeze-scales / --freeze-structure-factors (careless.py:48-56) and the non-finite-norm break (variational.py:271-274)"""
    kw = dict(N=300, R=40, d0=5, L=2, w=32, S=1)
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    model = util.build_model(data, cfg, params, 2, 32)
    inputs = util.reference_inputs(data)
    model.scaling_model.trainable = False
    w0 = model.scaling_model.mlp_scaler.flat.clone()
    model.train_model(inputs, 3, progress=False)
    assert torch.equal(model.scaling_model.mlp_scaler.flat.cpu(), w0.cpu())              # scaler frozen
    assert not torch.equal(model.surrogate_posterior.loc_raw.cpu(), torch.as_tensor(params.q_loc_raw.numpy().astype(np.float32)))
    model.scaling_model.trainable = True
    model.surrogate_posterior.trainable = False
    q0 = model.surrogate_posterior.loc_raw.clone()
    model.train_model(inputs, 2, progress=False)
    assert torch.equal(model.surrogate_posterior.loc_raw, q0)
    assert not torch.equal(model.scaling_model.mlp_scaler.flat.cpu(), w0.cpu())
    # a NaN observation makes the gradient norm NaN at the first step: that step is recorded, later ones are not run
    bad = dict(data)
    bad["iobs"] = np.array(data["iobs"], copy=True)
    bad["iobs"][7] = np.nan
    model2 = util.build_model(bad, cfg, params, 2, 32)
    hist = model2.train_model(util.reference_inputs(bad), 120, progress=False)
    assert len(hist["loss"]) == 1 and not np.isfinite(hist["Grad Norm"][0])
    assert bool(torch.isfinite(model2.surrogate_posterior.loc_raw).all())               # non-finite grads were zeroed (:208)


@pytest.mark.parametrize("kw", [dict(N=517, R=41, d0=5, L=2, w=32, S=3),
                                dict(N=600, R=50, L=2, w=32, S=2, laue=True),
                                dict(N=500, R=60, d0=5, L=2, w=32, S=2, double_wilson=True),
                                dict(N=700, R=40, d0=5, L=2, w=32, S=2, n_images=5, image_layers=1),
                                dict(N=600, R=40, d0=5, L=12, w=32, S=2),
                                dict(N=600, R=50, L=2, w=32, S=2, laue=True, image_layers=1, n_images=4),
                                dict(N=900, R=40, d0=5, L=20, w=10, S=2, perturb=0.02),
                                dict(N=700, R=40, d0=5, posenc=True, L=20, w=10, S=9, likelihood="studentt", dof=8.0, perturb=0.02),
                                dict(N=600, R=40, d0=5, L=2, w=32, S=3, ev11=True, likelihood="studentt", dof=6.0),
                                dict(N=500, R=60, d0=5, L=2, w=32, S=2, double_wilson=True, optimize_dw_r=True),
                                dict(N=600, R=40, d0=5, L=2, w=96, S=2),
                                dict(N=600, R=50, L=2, w=32, S=2, laue=True, ev11=True),
                                dict(N=700, R=40, d0=5, L=2, w=96, S=2, n_images=6, image_layers=1),
                                dict(N=900, R=40, d0=37, L=20, w=10, S=3, perturb=0.02)],
                         ids=["mono", "laue", "double_wilson", "image_layers", "chained_scaler", "laue_image_layers", "cli_default_20x10",
                              "cli_default_posenc_d21_S9", "ev11", "trainable_double_wilson_r", "wide_2x96", "laue_ev11", "wide_image_layers",
                              "peeled_first_layer_d37"])
@pytest.mark.parametrize("split", ["rows", "owners"])
def test_rank_shards_sum_to_full_batch_on_gpu(kw, split):
    """Data-parallel decomposition on ONE GPU: the engines of rank 0 and rank 1 of a 2-rank world (all-reduce skipped) produce
    partial losses / gradients that add up to the single-rank result; in-kernel noise is keyed by global indices, so the shards
    draw exactly the numbers the full batch draws.  `rows`: the row split (what every configuration runs at two ranks); `owners`:
    the reflection-owner split forced (monochromatic data with the Wilson prior: the default from four ranks on)."""
    from careless_amd.engine import ElboEngine, make_shard
    owner_eligible = not (kw.get("laue") or kw.get("double_wilson") or kw.get("image_layers") or kw["w"] > 64)
    if split == "owners" and not owner_eligible:
        pytest.skip("this configuration always runs the row split")
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    if kw.get("laue"):                                  # rows of a harmonic group are not contiguous in real inputs
        perm = np.random.default_rng(1).permutation(kw["N"])
        for k in ("refl_id", "image_id", "file_id", "metadata", "wavelength", "harmonic_id"):
            data[k] = np.asarray(data[k])[perm]
    inputs = util.reference_inputs(data)
    L, w = kw["L"], kw["w"]
    full = ElboEngine(util.build_model(data, cfg, params, L, w), inputs, seed=99)
    full.forward_backward(3)
    torch.cuda.synchronize()
    g_full, t_full = full.grads.clone(), full.loss_terms()
    g_sum, nll, kl = torch.zeros_like(g_full), 0.0, 0.0
    for r in range(2):
        m = util.build_model(data, cfg, params, L, w)
        if split == "owners":
            m.owner_shard = True
        eng = ElboEngine(m, inputs, seed=99, shard=make_shard(kw["N"], kw["R"], r, 2))
        assert eng.owner == (split == "owners")
        eng.local_only = True
        eng.forward_backward(3)
        torch.cuda.synchronize()
        g_sum += eng.grads
        t = eng.loss_terms()
        nll += t["nll"]; kl += t["kl"]
    assert abs(nll - t_full["nll"]) <= 1e-5 * abs(t_full["nll"]) and abs(kl - t_full["kl"]) <= 1e-5 * max(abs(t_full["kl"]), 1.0)
    assert util.rel_err(g_sum.cpu().numpy(), g_full.cpu().numpy()) < 2e-5


@pytest.mark.parametrize("workload", ["mono_10M_cli_default_20x10_S1", "mono_10M_studentt_posenc4_20x10_S8"], ids=["d5", "four_encoded_keys_d37_peeled"])
@pytest.mark.parametrize("owner", [True, False], ids=["reflection_owners", "rows"])
def test_full_size_rank_shards_of_the_cli_default_scaler_sum_to_the_full_batch(owner, workload):
    """1 M observations on the careless CLI's default scaler (20 x 10: the narrow kernel instance), in-kernel noise: the eight
    rank shards of an 8-GPU job -- reflection-owner split and row split --, run one after the other on this GPU without the
    all-reduce, add up to the single-GPU step: a size-independent property (every workgroup walks dozens of tiles, the accumulators
    carry over in registers and LDS).  Also with four positionally encoded keys (37 columns, 8 samples: the peeled first layer's
    kernels walk every shard's rows, round 5)."""
    from careless_amd.engine import ElboEngine, make_shard
    from careless_amd.workloads import make_workload
    model, inputs, data, spec = make_workload(workload, N=1_000_000)
    model.owner_shard = owner
    n, r = 1_000_000, int(model.surrogate_posterior.loc_raw.numel())
    full = ElboEngine(model, inputs, seed=7)
    full.forward_backward(1)
    torch.cuda.synchronize()
    g_full, t_full = full.grads.clone(), full.loss_terms()
    g_sum, nll, kl = torch.zeros_like(g_full), 0.0, 0.0
    for rank in range(8):
        eng = ElboEngine(model, inputs, seed=7, shard=make_shard(n, r, rank, 8))
        assert eng.owner == owner
        eng.local_only = True
        eng.forward_backward(1)
        torch.cuda.synchronize()
        g_sum += eng.grads
        t = eng.loss_terms()
        nll += t["nll"]; kl += t["kl"]
        del eng
    assert abs(nll - t_full["nll"]) <= 1e-6 * abs(t_full["nll"]) and abs(kl - t_full["kl"]) <= 1e-6 * max(abs(t_full["kl"]), 1.0)
    lay = full.layout
    for lo, hi in zip(lay.seg_off[:-1], lay.seg_off[1:]):                      # per trainable tensor (fp32 atomics: summation order only)
        a, b = g_sum[lo:hi], g_full[lo:hi]
        assert float((a - b).abs().max()) <= 2e-4 * max(float(b.abs().max()), 1e-6), (lo, hi)


@pytest.mark.parametrize("kw", [dict(N=1500, R=60, d0=5, L=5, w=64, S=3, likelihood="studentt", dof=8.0),
                                dict(N=1300, R=50, d0=5, posenc=True, L=20, w=10, S=2, perturb=0.02),
                                dict(N=1100, R=50, d0=5, L=12, w=32, S=2),
                                dict(N=1200, R=50, d0=41, L=20, w=10, S=2, perturb=0.02),
                                dict(N=1000, R=50, d0=5, posenc=True, L=9, w=12, S=2, perturb=0.03)],
                         ids=["mono_5x64", "cli_default_posenc_d21", "chained_12x32", "peeled_lane_d41", "peeled_narrow_9x12_d21"])
def test_shard_cut_into_several_launches_equals_one_launch(kw, monkeypatch):
    """A shard whose metadata image would pass 4 GiB runs as consecutive launches (engine.ObsChunks; the reference is full-batch at
    any N, variational.py:255-256).  With the bound lowered to a few hundred rows the same problem runs as 4 - 6 launches: loss,
    predictions and every gradient equal the oracle's (injected noise) and, with in-kernel noise, the single-launch step's."""
    from careless_amd.engine import ElboEngine, ObsChunks
    L, w = kw["L"], kw["w"]
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    inputs = util.reference_inputs(data)
    d = np.asarray(data["metadata"]).shape[1]
    monkeypatch.setenv("CARELESS_HIP_MAX_LAUNCH_BYTES", str(4 * ((d + 3) // 4 * 4) * 300))
    model = util.build_model(data, cfg, params, L, w)
    ipred = model(inputs, u_f=u_f, eta=eta).cpu().numpy()
    eng = model._engine
    assert isinstance(eng.obs, ObsChunks) and len(eng.obs.children) >= 4 and sum(c.N for c in eng.obs.children) == kw["N"]
    torch.cuda.synchronize()
    out, grads = O.elbo_value_and_grads(params, x, cfg, torch.as_tensor(u_f, dtype=torch.float64), torch.as_tensor(eta, dtype=torch.float64))
    t = eng.loss_terms()
    assert abs(t["loss"] - float(out["loss"])) <= RTOL_LOSS * abs(float(out["loss"]))
    assert util.rel_err(ipred, out["ipred"].numpy()) < 1e-4
    _assert_grads([g.cpu().numpy() for g in eng.grad_tensors()], grads, (data, cfg, params, u_f, eta), "chunked")
    # in-kernel noise: the pieces draw what the single launch draws (keyed by the global row)
    cut = ElboEngine(util.build_model(data, cfg, params, L, w), inputs, seed=31)
    cut.forward_backward(2)
    monkeypatch.delenv("CARELESS_HIP_MAX_LAUNCH_BYTES")
    one = ElboEngine(util.build_model(data, cfg, params, L, w), inputs, seed=31)
    assert not isinstance(one.obs, ObsChunks)
    one.forward_backward(2)
    torch.cuda.synchronize()
    ta, tb = cut.loss_terms(), one.loss_terms()
    assert abs(ta["nll"] - tb["nll"]) <= 1e-6 * abs(tb["nll"]) and ta["kl"] == tb["kl"]
    assert util.rel_err(cut.grads.cpu().numpy(), one.grads.cpu().numpy()) < 2e-5
    # and the training loop with validation data runs on the cut shard
    m2 = util.build_model(data, cfg, params, L, w)
    monkeypatch.setenv("CARELESS_HIP_MAX_LAUNCH_BYTES", str(4 * ((d + 3) // 4 * 4) * 300))
    tr, te = tuple(a[:900] for a in inputs), tuple(a[900:] for a in inputs)
    h = m2.train_model(tr, 3, progress=False, validation_data=te, validation_frequency=1)
    assert len(h["loss"]) == 3 and all(np.isfinite(h["loss"])) and all(np.isfinite(h["NLL_val"]))


@pytest.mark.parametrize("kw", [dict(N=1500, R=60, d0=5, L=5, w=64, S=3, likelihood="studentt", dof=8.0, n_images=7),
                                dict(N=900, R=50, d0=5, L=20, w=10, S=2, perturb=0.02),
                                dict(N=1300, R=40, d0=5, posenc=True, L=3, w=32, S=8, shuffle_rows=True, n_images=9),
                                dict(N=700, R=40, d0=5, L=2, w=32, S=1, use_image_scales=False, kl_weight=0.5),
                                # the default scaler keeps its own kernels in this mode (round 4): lane = observation with the metadata in
                                # registers / as LDS rows (positional encodings), more samples than a batch, the narrow kernel at other depths
                                dict(N=1100, R=50, d0=5, posenc=True, L=20, w=10, S=8, perturb=0.02, likelihood="studentt", dof=6.0, n_images=6),
                                dict(N=1000, R=40, d0=5, L=20, w=8, S=11, perturb=0.02, n_images=5),
                                dict(N=900, R=50, d0=5, L=6, w=10, S=5, perturb=0.03, likelihood="studentt", dof=6.0),
                                dict(N=800, R=40, d0=12, L=9, w=13, S=1, perturb=0.03, n_images=7),
                                # single-pass Laue on the default scaler's kernels (packed layout: stores by the caller's row)
                                dict(N=900, R=50, L=20, w=10, S=3, laue=True, perturb=0.02),
                                dict(N=700, R=40, L=4, w=12, S=2, laue=True, perturb=0.03, likelihood="studentt", dof=8.0),
                                # ... and on the 64- / 32-wide fused kernel (the packed deterministic compilation of elbo_mlp.hip)
                                dict(N=900, R=50, L=5, w=64, S=3, laue=True),
                                dict(N=700, R=40, L=3, w=32, S=9, laue=True, likelihood="studentt", dof=8.0, extra_meta=14),
                                # the double-Wilson prior (fixed r): parents pull their children's terms in list order
                                dict(N=800, R=60, d0=5, L=5, w=64, S=3, double_wilson=True),
                                dict(N=900, R=50, d0=5, L=20, w=10, S=2, double_wilson=True, perturb=0.02, likelihood="studentt", dof=8.0),
                                # scalers wider than 64 (round 4): the layer-by-layer path's one kernel with float atomics -- the slot
                                # likelihood of monochromatic rows -- stores per (row, sample) instead; everything else sums partials in order
                                dict(N=1500, R=60, d0=5, L=3, w=128, S=4, likelihood="studentt", dof=8.0, n_images=7),
                                dict(N=900, R=50, d0=5, L=2, w=96, S=2, use_image_scales=False),
                                # scalers deeper than one launch: the chain's last block is the launch with the epilogue
                                dict(N=900, R=50, d0=5, L=12, w=64, S=3, likelihood="studentt", dof=8.0, n_images=6),
                                dict(N=700, R=40, d0=5, L=25, w=10, S=2, perturb=0.02),
                                # the Evans-2011 error model: its three gradients leave as per-wave stores (cl_mlp_args / cl_laue_args.ev11_part)
                                dict(N=900, R=50, d0=5, L=5, w=64, S=3, ev11=True),
                                dict(N=900, R=50, d0=5, L=20, w=10, S=2, ev11=True, perturb=0.02),
                                dict(N=800, R=40, d0=5, L=6, w=10, S=5, ev11=True, perturb=0.03, likelihood="studentt", dof=8.0),
                                dict(N=700, R=40, L=3, w=32, S=2, laue=True, ev11=True),
                                dict(N=900, R=50, d0=5, L=2, w=80, S=4, ev11=True),
                                # a peeled first layer (round 5): its weight gradient sums per-workgroup partials in index order
                                dict(N=1100, R=50, d0=41, L=20, w=10, S=3, likelihood="studentt", dof=8.0, perturb=0.02, n_images=6),
                                dict(N=900, R=50, d0=5, L=12, w=16, S=3, perturb=0.02),
                                # per-image layers on the lane kernel's instances (round 6): one wave holds all tiles of an image
                                dict(N=1200, R=50, d0=5, L=20, w=10, S=2, n_images=7, image_layers=2, perturb=0.03),
                                dict(N=1000, R=50, d0=7, L=10, w=9, S=3, n_images=6, image_layers=1, ev11=True, perturb=0.03, likelihood="studentt", dof=8.0),
                                dict(N=1300, R=50, d0=5, posenc=True, L=20, w=10, S=2, n_images=8, image_layers=2, perturb=0.03),
                                dict(N=900, R=60, L=20, w=10, S=2, laue=True, n_images=6, image_layers=1, perturb=0.03),
                                dict(N=2600, R=60, d0=5, L=6, w=10, S=9, n_images=3, image_layers=2, perturb=0.03, shuffle_rows=True),
                                dict(N=1200, R=50, d0=5, L=20, w=10, S=2, n_images=7, image_layers=3, perturb=0.02),
                                dict(N=1200, R=50, d0=5, L=9, w=10, S=3, n_images=7, image_layers=3, perturb=0.03)],
                         ids=["mono_5x64", "cli_default_20x10", "rows_in_arbitrary_order_S8", "no_image_scales_klweight",
                              "lane_posenc_d21_S8", "lane_20x8_S11", "narrow_6x10_S5", "narrow_9x13_d12", "laue_lane_20x10_S3", "laue_narrow_4x12", "laue_5x64_S3", "laue_3x32_d20_S9",
                              "double_wilson_5x64", "double_wilson_lane_20x10", "wide_3x128_S4", "wide_2x96_noimg", "deep_12x64_S3", "deep_25x10",
                              "ev11_5x64", "ev11_lane_20x10", "ev11_narrow_6x10_S5", "ev11_laue_3x32", "ev11_wide_2x80_S4", "peel_20x10_d41_S3", "w16_12x16_S3",
                              "image_layers2_lane_20x10", "image_layers1_lane_10x9_ev11", "image_layers2_lane_peeled_d21", "laue_image_layers1_lane_20x10",
                              "image_layers2_lane_6x10_S9_three_large_images", "image_layers3_lane_20x10", "image_layers3_lane_9x10"])
def test_deterministic_mode_matches_oracle_and_repeats_bit_for_bit(kw, monkeypatch):
    """`model.deterministic = True` (or CARELESS_HIP_DETERMINISTIC=1): the fused kernel stores per-observation contributions instead of
    issuing float atomics and `cl_det_reduce` sums them in row order (include/careless_hip.h).  Same parity bar against the oracle,
    and two engines on the same inputs produce bit-identical gradients, loss terms and -- after several Adam steps -- parameters;
    also with the shard cut into several launches."""
    from careless_amd.engine import ElboEngine
    kw = dict(kw)
    shuffle = kw.pop("shuffle_rows", False)
    L, w = kw["L"], kw["w"]
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    if shuffle:
        perm = np.random.default_rng(2).permutation(kw["N"])
        for k in ("refl_id", "image_id", "file_id", "metadata", "iobs", "sigiobs"):
            data[k] = np.asarray(data[k])[perm]
        eta = eta[:, perm]
        x = O.inputs_from_numpy(data)
    inputs = util.reference_inputs(data)

    def fresh():
        m = util.build_model(data, cfg, params, L, w)
        m.deterministic = True
        return m
    model = fresh()
    ipred = model(inputs, u_f=u_f, eta=eta).cpu().numpy()
    eng = model._engine
    assert eng.deterministic and "deterministic" in eng.kernel_name()
    torch.cuda.synchronize()
    out, grads = O.elbo_value_and_grads(params, x, cfg, torch.as_tensor(u_f, dtype=torch.float64), torch.as_tensor(eta, dtype=torch.float64))
    t = eng.loss_terms()
    assert abs(t["loss"] - float(out["loss"])) <= RTOL_LOSS * abs(float(out["loss"]))
    assert util.rel_err(ipred, out["ipred"].numpy()) < 1e-4
    _assert_grads([g.cpu().numpy() for g in eng.grad_tensors()], grads, (data, cfg, params, u_f, eta), "deterministic")
    runs = []
    for cut in (False, False, True):
        if cut and (kw.get("laue") or w > 64 or kw.get("image_layers")):
            break                                   # (packed layouts and the layer-by-layer path are not cut into launches)
        if cut:
            d = np.asarray(data["metadata"]).shape[1]
            monkeypatch.setenv("CARELESS_HIP_MAX_LAUNCH_BYTES", str(4 * ((d + 3) // 4 * 4) * 400))
        e = ElboEngine(fresh(), inputs, seed=5)
        e.forward_backward(1)
        torch.cuda.synchronize()
        g, terms = e.grads.clone(), e.loss_terms()
        e.alloc_history(4)
        for i in range(4):
            e.train_step(i)
        torch.cuda.synchronize()
        runs.append((g, terms, e.params.clone(), e.read_history(4)))
    (g0, t0, p0, h0), (g1, t1, p1, h1) = runs[:2]
    assert torch.equal(g0, g1) and t0["nll"] == t1["nll"] and torch.equal(p0, p1) and h0["NLL"] == h1["NLL"]
    if len(runs) < 3:
        return
    g2, t2, p2, h2 = runs[2]
    # cut into launches: the per-reflection / per-image sums still run in row order -> the same bits in dz_f and the image scales; the
    # scaler's weight gradient adds the pieces' partials in a different grouping (same values to rounding)
    assert util.rel_err(g2.cpu().numpy(), g0.cpu().numpy()) < 2e-5
    # (the last piece may hold fewer tiles than the first: every piece's NLL slots are counted, none twice)
    assert abs(t2["nll"] - t0["nll"]) <= 1e-6 * abs(t0["nll"]) and np.allclose(h2["NLL"], h0["NLL"], rtol=1e-6)


def test_flip_resolutions_stay_rare():
    """Runs after the parity cases of this module (pytest keeps file order): the forced-branch resolution is for measure-zero events,
    not a habit -- a handful of cases among the few hundred at most."""
    assert len(FLIP_CASES) <= 6, FLIP_CASES


# --------------------------------------------------------------------------------------------------------------------------
# reflection-owner data parallelism: a rank takes a range of reflections and every observation of theirs
# --------------------------------------------------------------------------------------------------------------------------
OWNER_CASES = {
    "mono_2x32": dict(N=517, R=41, d0=5, L=2, w=32, S=3),
    "headline_shape_5x64_posenc_S8": dict(N=900, R=60, d0=5, posenc=True, L=5, w=64, S=8, likelihood="studentt", dof=16.0),
    "cli_default_20x10": dict(N=900, R=40, d0=5, L=20, w=10, S=2, perturb=0.02),
    "cli_default_posenc_d21_S9": dict(N=700, R=40, d0=5, posenc=True, L=20, w=10, S=9, likelihood="studentt", dof=8.0, perturb=0.02),
    "narrow_20x13": dict(N=800, R=40, d0=5, L=20, w=13, S=2, perturb=0.02),
    "chained_12x32": dict(N=600, R=40, d0=5, L=12, w=32, S=2),
    "ev11": dict(N=600, R=40, d0=5, L=2, w=32, S=3, ev11=True, likelihood="studentt", dof=6.0),
    "klweight_noimg": dict(N=500, R=40, d0=5, L=3, w=20, S=2, kl_weight=0.5, use_image_scales=False),
    "global_clipnorm": dict(N=400, R=40, d0=5, L=2, w=32, S=2, global_clipnorm=1.0),
    "clipnorm": dict(N=400, R=40, d0=5, L=2, w=32, S=2, clipnorm=0.5),
}


@pytest.mark.parametrize("name", list(OWNER_CASES))
@pytest.mark.parametrize("world", [2, 3])
def test_reflection_owner_shards_reproduce_the_full_batch_step(name, world):
    """The engines of all ranks of a reflection-owner split, run one after the other on this GPU with the all-reduce replaced by a
    sum of their messages: loss terms and gradients add up to the single-rank step's (in-kernel noise: keyed by the GLOBAL row and
    reflection, so the shards draw what the full batch draws), and after the optimizer step the owners' a / b and everybody's copy
    of the replicated tail equal the single-rank parameters; the logged gradient norm is the full-batch one on every rank."""
    from careless_amd.engine import ElboEngine, make_shard
    kw = OWNER_CASES[name]
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    inputs = util.reference_inputs(data)
    L, w, R = kw["L"], kw["w"], kw["R"]
    full = ElboEngine(util.build_model(data, cfg, params, L, w), inputs, seed=99)
    full.alloc_history(1)
    full.forward_backward(0)
    torch.cuda.synchronize()
    g_full, t_full = full.grads.clone(), full.loss_terms()
    full.optimizer_step(0)
    h_full = full.read_history(1)
    engs = []
    for r in range(world):
        m = util.build_model(data, cfg, params, L, w)
        m.owner_shard = True                    # (the automatic choice takes the owner split from four ranks on)
        eng = ElboEngine(m, inputs, seed=99, shard=make_shard(kw["N"], R, r, world))
        assert eng.owner and eng.shard.owner and eng.shard.rank == r
        eng.local_only = True
        eng.alloc_history(1)
        eng.forward_backward(0)
        engs.append(eng)
    torch.cuda.synchronize()
    # the shards partition reflections and rows
    rows = np.concatenate([e.shard.rows for e in engs])
    assert len(rows) == kw["N"] and len(np.unique(rows)) == kw["N"]
    assert engs[0].shard.kl_begin == 0 and engs[-1].shard.kl_end == R and all(a.shard.kl_end == b.shard.kl_begin for a, b in zip(engs, engs[1:]))
    g_sum = sum(e.grads for e in engs)
    nll, kl = sum(e.loss_terms()["nll"] for e in engs), sum(e.loss_terms()["kl"] for e in engs)
    assert abs(nll - t_full["nll"]) <= 1e-5 * abs(t_full["nll"]) and abs(kl - t_full["kl"]) <= 1e-5 * max(abs(t_full["kl"]), 1.0)
    assert util.rel_err(g_sum.cpu().numpy(), g_full.cpu().numpy()) < 2e-5
    for e in engs:                                   # a rank's q gradient lives on its own reflections only
        own = torch.zeros(2 * R, dtype=torch.bool)
        own[e.shard.kl_begin:e.shard.kl_end] = True
        own[R + e.shard.kl_begin:R + e.shard.kl_end] = True
        assert float(e.grads[:2 * R][~own.to(e.grads.device)].abs().max()) == 0.0
    # the all-reduce: every rank gets the sum of the messages (scaler gradient + the four norm terms)
    msg = sum(e.msg for e in engs).clone()
    for e in engs:
        e.msg.copy_(msg)
        e.optimizer_step(0)
    torch.cuda.synchronize()
    p_full = full.params.cpu().numpy()
    for e in engs:
        p = e.params.cpu().numpy()
        r0, r1 = e.shard.kl_begin, e.shard.kl_end
        for lo, hi in ((r0, r1), (R + r0, R + r1), (2 * R, len(p))):
            assert util.rel_err(p[lo:hi], p_full[lo:hi]) < 2e-5, (e.shard.rank, lo, hi)
        h = e.read_history(1)
        assert abs(h["Grad Norm"][0] - h_full["Grad Norm"][0]) <= 2e-5 * h_full["Grad Norm"][0]
    # the others' reflections were not touched (they arrive with sync_owned at the end of training)
    p0 = engs[0].params.cpu().numpy()
    init = np.concatenate([params.q_loc_raw.numpy(), params.q_scale_raw.numpy()]).astype(np.float32)
    r1 = engs[0].shard.kl_end
    assert np.array_equal(p0[r1:R], init[r1:R])


def test_reflection_owner_shards_with_injected_noise_match_the_oracle():
    """Owner shards on injected noise (the columns of eta follow the shard's rows): the summed loss and gradients equal the fp64
    oracle's, so the decomposition is checked against the reference restatement and not only against the engine itself; the
    validation NLL of an owner-sharded validation set sums to the single-rank value."""
    from careless_amd.engine import ElboEngine, make_shard
    kw = dict(N=640, R=48, d0=5, L=5, w=64, S=4, likelihood="studentt", dof=8.0)
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    inputs = util.reference_inputs(data)
    out, grads = O.elbo_value_and_grads(params, x, cfg, torch.as_tensor(u_f, dtype=torch.float64), torch.as_tensor(eta, dtype=torch.float64))
    full = ElboEngine(util.build_model(data, cfg, params, 5, 64), inputs, seed=5)
    vfull = full.evaluate_nll(full.make_obs(inputs), 77)
    gs, nll, kl, vsum = None, 0.0, 0.0, 0.0
    for r in range(3):
        m = util.build_model(data, cfg, params, 5, 64)
        m.owner_shard = True
        eng = ElboEngine(m, inputs, seed=5, shard=make_shard(kw["N"], kw["R"], r, 3))
        assert eng.owner
        eng.local_only = True
        du, de = eng._noise_to_device(u_f, eta)
        eng.forward_backward(0, du, de)
        torch.cuda.synchronize()
        gt = [g.clone() for g in eng.grad_tensors()]
        gs = gt if gs is None else [a + b for a, b in zip(gs, gt)]
        t = eng.loss_terms()
        nll += t["nll"]; kl += t["kl"]
        vsum += eng.evaluate_nll(eng.make_obs(inputs), 77)
    assert abs(nll - float(out["nll"])) <= 1e-4 * abs(float(out["nll"])) and abs(kl - float(out["kl"])) <= 1e-4 * abs(float(out["kl"]))
    for a, b in zip(gs, grads):
        assert util.rel_err(a.cpu().numpy(), b.numpy()) < 2e-4
    assert abs(vsum - vfull) <= 1e-5 * abs(vfull)


def test_reflection_owner_shard_cut_into_several_launches(monkeypatch):
    """An owner shard whose metadata would pass the 4-GiB bound of a launch runs as consecutive launches like any other shard
    (engine.ObsChunks over the shard's row list): with the bound lowered to a few hundred rows, the ranks' gradients -- in-kernel
    noise keyed by the global row, injected noise picked by it -- still add up to the single-rank, single-launch step."""
    from careless_amd.engine import ElboEngine, ObsChunks, make_shard
    kw = dict(N=1400, R=60, d0=5, posenc=True, L=5, w=64, S=3, likelihood="studentt", dof=8.0)
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    inputs = util.reference_inputs(data)
    full = ElboEngine(util.build_model(data, cfg, params, 5, 64), inputs, seed=11)
    full.forward_backward(2)
    torch.cuda.synchronize()
    g_full, t_full = full.grads.clone(), full.loss_terms()
    out, grads = O.elbo_value_and_grads(params, x, cfg, torch.as_tensor(u_f, dtype=torch.float64), torch.as_tensor(eta, dtype=torch.float64))
    d = np.asarray(data["metadata"]).shape[1]
    monkeypatch.setenv("CARELESS_HIP_MAX_LAUNCH_BYTES", str(4 * ((d + 3) // 4 * 4) * 256))        # 256 rows per launch
    g_sum, nll, gs = torch.zeros_like(g_full), 0.0, None
    for r in range(2):
        m = util.build_model(data, cfg, params, 5, 64)
        m.owner_shard = True
        eng = ElboEngine(m, inputs, seed=11, shard=make_shard(kw["N"], kw["R"], r, 2))
        assert eng.owner and isinstance(eng.obs, ObsChunks) and len(eng.obs.children) >= 2
        eng.local_only = True
        eng.forward_backward(2)
        torch.cuda.synchronize()
        g_sum += eng.grads
        nll += eng.loss_terms()["nll"]
        du, de = eng._noise_to_device(u_f, eta)
        eng.forward_backward(0, du, de)
        torch.cuda.synchronize()
        gt = [g.clone() for g in eng.grad_tensors()]
        gs = gt if gs is None else [a + b for a, b in zip(gs, gt)]
    assert abs(nll - t_full["nll"]) <= 1e-5 * abs(t_full["nll"])
    assert util.rel_err(g_sum.cpu().numpy(), g_full.cpu().numpy()) < 2e-5
    for a, b in zip(gs, grads):
        assert util.rel_err(a.cpu().numpy(), b.numpy()) < 2e-4


# seeded random sweep over what the reflection-owner split takes: monochromatic configurations of the engine sweep above, cut over a
# random number of ranks (OWNER_RANDOM_N=60 OWNER_RANDOM_SEED=5 python -m pytest tests/test_gpu_parity.py -k random_owner)
def _random_owner_cases(n, seed):
    pool = {k: v for k, v in _random_engine_cases(6 * n + 12, seed).items() if "_mono_" in k and v["w"] <= 64 and v["R"] >= 12}
    rng = np.random.default_rng(seed + 1)
    out = {}
    for k, v in list(pool.items())[:n]:
        out[f"{k}_ranks{int(rng.integers(2, 6))}"] = v
    return out


RANDOM_OWNER_CASES = _random_owner_cases(int(os.environ.get("OWNER_RANDOM_N", "6")), int(os.environ.get("OWNER_RANDOM_SEED", "21")))


@pytest.mark.parametrize("name", list(RANDOM_OWNER_CASES))
def test_random_owner_shards_match_the_oracle(name):
    """The ranks' loss terms and gradients of a reflection-owner split, on injected noise, add up to the fp64 oracle's (same gate as
    every other case: 2e-4 on every tensor)."""
    from careless_amd.engine import ElboEngine, make_shard, owner_bounds
    kw = dict(RANDOM_OWNER_CASES[name])
    world = int(name.rsplit("ranks", 1)[1])
    shuffle, grid = kw.pop("shuffle_rows", False), kw.pop("grid", None)
    L, w = kw["L"], kw["w"]
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    if shuffle:
        perm = np.random.default_rng(2).permutation(kw["N"])
        for k in ("refl_id", "image_id", "file_id", "metadata", "iobs", "sigiobs"):
            data[k] = np.asarray(data[k])[perm]
        eta = eta[:, perm]
        x = O.inputs_from_numpy(data)
    if owner_bounds(np.asarray(data["refl_id"]), kw["R"], world) is None:
        pytest.skip("fewer observed reflections than ranks: the engine keeps the row split")
    out, grads = O.elbo_value_and_grads(params, x, cfg, torch.as_tensor(u_f, dtype=torch.float64), torch.as_tensor(eta, dtype=torch.float64))
    inputs = util.reference_inputs(data)
    gs, nll, kl = None, 0.0, 0.0
    for r in range(world):
        m = util.build_model(data, cfg, params, L, w)
        m.owner_shard, m.kernel_grid = True, grid
        eng = ElboEngine(m, inputs, seed=3, shard=make_shard(kw["N"], kw["R"], r, world), grid=grid)
        assert eng.owner
        eng.local_only = True
        du, de = eng._noise_to_device(u_f, eta)
        eng.forward_backward(0, du, de)
        torch.cuda.synchronize()
        gt = [g.cpu().numpy().copy() for g in eng.grad_tensors()]
        gs = gt if gs is None else [a + b for a, b in zip(gs, gt)]
        t = eng.loss_terms()
        nll += t["nll"]; kl += t["kl"]
    assert abs(nll - float(out["nll"])) <= RTOL_LOSS * abs(float(out["nll"])) and abs(kl - float(out["kl"])) <= RTOL_LOSS * max(abs(float(out["kl"])), 1.0)
    _assert_grads(gs, grads, (data, cfg, params, u_f, eta), name)
