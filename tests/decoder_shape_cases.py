"""The case lists of tests/test_gpu_decoder_shapes.py, shared with tests/test_decoder_shapes_cpu.py (plain data, no GPU).

The reference's evaluation script lists six narrow decoders: z_dim 16 or 32 over h_dim [128] or [128, 128].  The sweeps
over F, K and R run at 32 / [128, 128]; here the other three shapes cross the bin counts at which the dispatch changes.
The decoder's shape does not enter the dispatch, so each kernel form meets each shape only through this cross.
Every case runs on the ragged batch dispatch_model.COUNTS."""

# (z_dim, h_dim as the reference names it)
D = [(16, (128,)), (32, (128,)), (16, (128, 128))]
D_IDS = ["z16_h128", "z32_h128", "z16_h128x128"]

# bf16x3 mode, K = 10, R = 10: F -> the kernel forms it reaches by the restated dispatch
X3_F = {17: "wchain<5> with the odd bin; team geometry 0 with one tile under VAENMF_TEAM_CHAIN=1",
        80: "wchain<5,exact>: five tiles, lo fragments in LDS, no odd bin",
        81: "wchain<17>: lo fragments from L2",
        257: "wchain<17,exact>; team geometry 3 under VAENMF_TEAM_CHAIN=1",
        273: "team by default, geometry 0",
        513: "team geometry 4, the reference's shape",
        640: "team geometry 2, Fs == F"}
X3_K, X3_R = 10, 10
# bf16 mode, K = 8, R = 10
BF16_F = {9: "wchain<5>, one partial tile; group W statistics",
          201: "wchain<17>; group W statistics",
          257: "wchain4<17> (wchain<17,exact> under VAENMF_WCHAIN4=0) with the group W statistics",
          513: "wchain4<33> (wchain<33,GT33> under VAENMF_WCHAIN4=0); team geometry 4",
          529: "team by default: geometry 2, 33 tiles and the odd bin",
          640: "team geometry 2, Fs == F"}
BF16_K, BF16_R = 8, 10

X3_CASES = [(F, d) for F in X3_F for d in range(len(D))]
BF16_CASES = [(F, d) for F in BF16_F for d in range(len(D))]
# labels: (decoder shape, F, precision, Dy); Dy = F is the width of the reference's IBM labels
LABEL_CASES = [(d, F, prec, Dy) for d in (0, 2) for F in (65, 257) for prec in ("bf16x3", "bf16") for Dy in (1, F)]
# fixed noise PSD (gains only): (32, [128]), bf16x3
NOISE_PSD_F = [257, 513]
# latent padding at z_dim 16: (F, precision, the chain kernel the case is about)
PADDING_CASES = [(81, "bf16x3", 1), (257, "bf16", 2), (273, "bf16x3", 0)]
PADDING_D = [0, 2]
# fused run: one (F, precision, decoder shape) per chain kernel
RUN_CASES = [(81, "bf16x3", 0), (257, "bf16", 0), (513, "bf16x3", 1)]


def case_id(F, d):
    return "f%d_%s" % (F, D_IDS[d])


def chain_cases():
    """Every (F, K, R, decoder shape, precision) whose replayed chain the GPU helpers compare with the oracle's."""
    return [(F, X3_K, X3_R, d, "bf16x3") for F, d in X3_CASES] + [(F, BF16_K, BF16_R, d, "bf16") for F, d in BF16_CASES]
