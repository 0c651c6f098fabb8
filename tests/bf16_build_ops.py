"""Which GEMMs of the bf16 throughput build (libdopamine_amd_bf16.so: -DDQ_CNN_X6=1
-DDQ_X6_PAIRS=1) run on the bf16 matrix instruction, read off the tile template arguments in
dopamine_amd/csrc/nature_cnn.hip and iqn.hip, as data: tests/test_gpu_bf16_build.py holds the
device to it in both directions and tests/test_bf16_reference_cpu.py checks the measure on it.
A wave-private tile (Tile<1, 1, WK>, WK > 1) is bf16 under DQ_CNN_X6=1 (cnn_x6), every
gemm_iqn (kIqnX6) is bf16 in every build and one product under DQ_X6_PAIRS=1; every other
tile is the product's exact fp32."""

# (B, n_out): the ragged and degenerate cases of tests/test_gpu_cnn_layers.py
CNN_CASES = ((33, 918), (5, 129), (1, 1))
# (B, nq, A, E) from oracle/iqn_head.CASES: R = 1; fused, E = 4; fused, ragged second row tile;
# unfused with the wide dWe; unfused with the ragged E = 68 K slice
IQN_CASES = ((1, 1, 1, 64), (3, 4, 4, 4), (17, 8, 18, 64), (27, 5, 3, 64), (11, 3, 4, 68))
# key of oracle/nature_cnn.layer_reference's dict -> what it is called
PARTS = (('z', 'forward'), ('dx', 'input grad'), ('dw', 'weight grad'), ('db', 'bias grad'))


def cnn_is_bf16(layer, key):
  """The fc weight-gradient tiles (gemm<4, 4, 1> over [in | 1], so their bias gradients too)
  are block-shared and stay exact fp32; every other Nature-CNN GEMM is wave-private."""
  return not (layer in ('fc1', 'fc2') and key in ('dw', 'db'))


def iqn_bf16_stages(nq):
  """The head's stages on the bf16 instruction.  dW2|db2 (gemm<1, 4, 4>) and dX (kDxX6 false:
  dpre, dtl, dstate) are exact fp32.  dbe is the ones column of the wide dWe GEMM only when
  the dX epilogue is not fused (128 % nq != 0); fused, it is the exact fp32 sum of the
  epilogue's column partials (k_colsum) and the narrow dWe GEMM has no ones column."""
  fused = 128 % nq == 0
  return ('emb', 'h', 'q', 'dh', 'dw1', 'db1', 'dwe') + (() if fused else ('dbe',))
