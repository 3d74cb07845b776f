"""The library's dispatch and persistent loops, restated in plain Python (no torch, no library): which kernel form a
shape takes (shape_class, stream_class, decode_class, chain_form) and which frames / wave tiles / tiles a wavefront or
workgroup of a persistent kernel walks, trip by trip.  CPU tests check that the case lists of the GPU modules reach every
form with these; the GPU tests check the library's plan queries against them -- a later change of the dispatch makes a sweep
fail instead of silently uncovering a kernel."""
import numpy as np

COUNTS = [21, 40, 9]         # the ragged batch of the sweeps over F, K and R
N_WAVE_TILES = sum((n + 15) // 16 for n in COUNTS)


def shape_class(F, K, precision, n_wave_tiles, R=30, n_cus=256):
    """The dispatch of plan.hip (vaenmf_plan_create), chain.hip (vn_wchain_supported, vn_launch_wchain) and stream.hip
    (launch_stream, launch_st, w_fused_ok, w_group_ok) with every switch at its default.  n_wave_tiles: 16-frame groups
    of the batch; R: samples per frame of the stored M-step; n_cus: compute units of the device."""
    bf16 = precision == "bf16"
    Fs = (F + 15) // 16 * 16
    Fm = F - 1 if (F % 16 == 1 and F > 16) else F            # plan.hip: the odd last bin leaves the tiles
    Kp = 8 if K <= 8 else (16 if K <= 16 else 32)
    team_tiles = (Fm + 15) // 16
    geom = 3 if team_tiles == 16 else (0 if team_tiles <= 20 else (4 if team_tiles == 32 else 2))
    tiles = (F + 15) // 16                                   # the wave chain keeps every bin on the MFMA path
    if tiles > 17 and not (tiles == 33 and bf16):
        chain_kernel, chain_form = 0, "team"
    elif bf16 and tiles in (17, 33) and n_wave_tiles <= n_cus:
        chain_kernel, chain_form = 2, "wchain4<%d>" % tiles
    else:
        chain_kernel = 1
        chain_form = ("wchain<33,GT33>" if tiles == 33 else "wchain<17,exact>" if tiles == 17 else "wchain<5,exact>" if tiles == 5
                      else "wchain<5>" if tiles < 5 else "wchain<17>")
    nch = (Fm + 255) // 256
    w_fused = 0
    if bf16 and Kp == 8 and nch == 1 and R in (10, 30):
        w_fused = 2 if n_wave_tiles <= n_cus else 1
    return dict(Fs=Fs, Fm=Fm, Kp=Kp, chain_tiles=tiles, chain_kernel=chain_kernel, chain_form=chain_form,
                partial_tile=F % 16 != 0, lo_in_lds=(not bf16) and tiles <= 5, pair_tiles=((tiles - 1) & ~1) if bf16 else 0,
                team_tiles=team_tiles, geom=geom, nch=nch, tail=Fm % 4 != 0,
                w_in_lds=Kp <= 8 or Fs * Kp * 4 <= 72 * 1024, w_fused=w_fused)


def chain_form(F, precision, n_wave_tiles, K=10, R=10):
    """(kernel form with VAENMF_WCHAIN4=0 where the default is wchain4_kernel, whether that switch is needed).  K and R are
    those of the chain cases of tests/persistent_cases.py; the chain's dispatch depends on neither."""
    sc = shape_class(F, K, precision, n_wave_tiles, R)
    if sc["chain_kernel"] == 2:
        return shape_class(F, K, precision, n_wave_tiles, R, n_cus=0)["chain_form"], True
    return sc["chain_form"], False


# ---------------------------------------------------------------------------------------------------------------------
# The persistent loops, restated: which frames / wave tiles / tiles a wavefront or workgroup walks, trip by trip.  `cap` is
# VAENMF_GRID_CAP (0: none).  tests/test_persistent_loops_cpu.py checks what the capped cases reach with these.
def wave_tiles(counts):
    """plan.hip, vaenmf_bind_batch_async: the 16-frame wave tiles of a batch, [(utterance, first frame, frames)]."""
    off = np.concatenate([[0], np.cumsum(counts)])
    return [(u, int(n), int(min(16, off[u + 1] - n))) for u in range(len(counts)) for n in range(off[u], off[u + 1], 16)]


def decode_tiles(counts, geom):
    """plan.hip: the tiles of decode_kernel, 64 frames with two teams (geometries 0 and 3), else 32."""
    tf = 64 if geom in (0, 3) else 32
    off = np.concatenate([[0], np.cumsum(counts)])
    return [(u, int(n), int(min(tf, off[u + 1] - n))) for u in range(len(counts)) for n in range(off[u], off[u + 1], tf)]


def stream_grid(NT, n_cus, cap=0, pipelined=False):
    """stream.hip, launch_stream: workgroups (of four wavefronts) of the streaming kernels; pipelined: wstats_stream2_kernel."""
    grid = min((2 if pipelined else 4) * n_cus, (NT + 3) // 4)
    return cap if 0 < cap < grid else grid


def wave_frames(NT, grid, wpb=4):
    """stream.hip, wave_frames: (per, [(n_beg, n_end) per wavefront, workgroup-major]); n_beg >= n_end: no frames."""
    nw = grid * wpb
    per = (NT + nw - 1) // nw
    return per, [(gw * per, min(gw * per + per, NT)) for gw in range(nw)]


def chain_waves(precision, chain_tiles):
    """chain.hip, vn_launch_wchain: wavefronts of a wchain_kernel workgroup."""
    return 4 if (precision == "bf16x3" or chain_tiles == 33) else 8


def chain_grid(n_wave_tiles, n_cus, cap=0):
    """chain.hip, wc_launch_s."""
    grid = min(n_wave_tiles, n_cus)
    return cap if 0 < cap < grid else grid


def chain_rounds(n_wave_tiles, grid, nwaves):
    """chain.hip, wchain_kernel: {(workgroup, wavefront): [wave tile of round 0, 1, ..]}; tile (i nwaves + w) grid + b."""
    rounds = (n_wave_tiles + grid * nwaves - 1) // (grid * nwaves)
    return {(b, w): [wt for wt in ((i * nwaves + w) * grid + b for i in range(rounds)) if wt < n_wave_tiles]
            for b in range(grid) for w in range(nwaves)}, rounds


def decode_grid(n_tiles, n_cus, cap=0):
    """engine.hip, launch_decode."""
    grid = min(n_tiles, 2 * n_cus)
    return cap if 0 < cap < grid else grid


def decode_trips(n_tiles, grid):
    """engine.hip, decode_kernel: [tiles of workgroup b, in the order of its trips]."""
    return [list(range(b, n_tiles, grid)) for b in range(grid)]


# the default launch: no switch, sizes from the device's CU count
def default_stream_counts(n_cus, n_utt=40):
    """About n_utt ragged utterances with 16 n_cus + 41 frames in all: two frames per wavefront of the 4 n_cus workgroups, the
    last block clipped to one frame, the wavefronts behind it empty."""
    NT = 16 * n_cus + 41
    cuts = np.sort(np.random.default_rng(40).choice(np.arange(1, NT), n_utt - 1, replace=False))
    return [int(v) for v in np.diff(np.concatenate([[0], cuts, [NT]]))]


def default_chain_counts(n_cus):
    """8 n_cus + 52 utterances of 1..16 frames, one wave tile each: a second round of wchain_kernel's eight wavefronts."""
    return [1 + (7 * u) % 16 for u in range(8 * n_cus + 52)]


# ---------------------------------------------------------------------------------------------------------------------
# the streaming and decoding kernels over the rank K and the samples per frame R
def _row_class(R, RB, HB=0):
    """Which of a kernel's row loops a frame of R rows takes: within the first half batch, within one batch, several
    full batches, or a partial last batch."""
    if HB and R <= HB:
        return "half"
    if R <= (2 * HB if HB else RB):      # (wstats_stream: two half batches; an odd RB = 2 HB + 1 rows go through the batch loop)
        return "one"
    return "exact" if R % RB == 0 else "partial"


def stream_class(F, K, R, precision, variant, n_wave_tiles, n_cus=256, wfused=True, wgroup=True):
    """stream.hip: launch_stream / launch_kp / launch_one / launch_st, w_fused_ok, w_group_ok and the RowBatch sizes of
    wstats_stream_kernel, wstats_stream2_kernel, hg_stream_kernel and wf_stream_kernel.  variant: "M1", "M2" (labels) or
    "noNMF" (fixed noise PSD: gains only).  wfused / wgroup: the switches VAENMF_WFUSED / VAENMF_WGROUP.
    Returns {"wstats": .., "hg": .., "wf": ..}; "wstats" is None when only the gains move."""
    bf16 = precision == "bf16"
    store = "bf16" if bf16 else "float"
    Fs = (F + 15) // 16 * 16
    Fm = F - 1 if (F % 16 == 1 and F > 16) else F
    KP = 8 if K <= 8 else (16 if K <= 16 else 32)
    NCH = min((Fm + 255) // 256, 3)
    tail = Fm % 4 != 0
    base = (32 if bf16 else 16) // NCH                                    # RowBatch<NCH, ST>::RB
    common = dict(NCH=NCH, KP=KP, store=store, tail=tail, extra_bin=F != Fm, w_in_lds=KP <= 8 or Fs * KP * 4 <= 72 * 1024)

    def kind(name, RB, HB=0, TAIL=False, RT=0, **kw):
        return dict(common, kernel=name, RB=RB, HB=HB, TAIL=TAIL, RT=RT, rows=_row_class(R, RB, HB), **kw)

    gains_only = variant == "noNMF"
    if gains_only:
        ws = None
    elif bf16 and KP == 8 and NCH == 1 and R in (10, 30) and wfused:      # w_fused_ok; w_group_ok: a small batch
        ws = kind("wstats_group" if (n_wave_tiles <= n_cus and wgroup) else "wstats_fused", 32, RT=R)
    elif NCH == 1 and KP <= 8 and R <= base:
        ws = kind("wstats_stream2", base)
    else:
        ws = kind("wstats_stream", base, HB=base // 2)
    RT = 0
    if (NCH == 1 and KP <= 8 and R in (10, 30)) or (NCH == 2 and bf16 and KP == 16 and R == 30):
        RT = R                                                             # the exact-count forms (not with TAIL)
    RBhg = 32 if ((bf16 and NCH == 2 and KP <= 16) or (not bf16 and NCH == 1 and KP <= 8)) else base
    hg = kind("hg_stream", RBhg, TAIL=tail, RT=0 if tail else RT, rt_shape=RT, gains_only=gains_only)
    wf = kind("wf_stream", base, TAIL=tail)
    return dict(wstats=ws, hg=hg, wf=wf)


def decode_class(F, K, R, precision):
    """engine.hip: launch_decode (with_geom, then the rank) and decode_kernel's loop over chunks of 32 samples."""
    sc = shape_class(F, K, precision, N_WAVE_TILES)
    m = R % 32
    return dict(geom=sc["geom"], split=precision == "bf16x3", KP=sc["Kp"], chunks=(R + 31) // 32,
                rmod="0" if m == 0 else ("1..15" if m < 16 else ("16" if m == 16 else "17..31")), extra_bin=F != sc["Fm"])
