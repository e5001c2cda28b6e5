"""The host's plan for wg_policy_forward / wg_policy_backward restated (pr_check, pr_backward_plan and wg_policy_forward
in csrc/pg_hip.hip), and the shapes that sit on the plan's edges.  tests/test_policy_rows_cpu.py anchors the restatement
on wg_policy_backward_workspace, which plans without launching; tests/test_gpu_policy_rows.py launches every shape and
asserts from the restatement the property the shape is there for, so that a shape which drifts off its edge fails.
"""
THREADS = 256            # PR_THREADS
LDS = 64 * 1024          # PR_LDS
W_LDS = 32 * 1024        # PR_W_LDS: the forward stages a shared policy's weights up to this size
FWD_ROWS, BWD_ROWS = 64, 16
FWD_CAP, FWD_CAP_L2 = 2048, 1 << 20     # workgroups of the forward, staged / through L2
MAX_K = 16384            # WG_POLICY_GRAD_MAX_K


def up4(v):
    return (v + 3) & ~3


def plan(D, H, C, G=1, b1=True, b2=True, rows=1, layer1=True):
    """D, H, C, G and which biases exist -> the plan.  rows: n_steps * N (the forward's tile count); layer1=False: the
    backward call with g_w1 and g_b1 NULL (T1 = 0)."""
    b1 = bool(b1 and H)
    n2 = H or D
    K = D * H + (H if b1 else 0) + n2 * C + (C if b2 else 0)
    # the backward: 4 x 4 register blocks of (x|1) (x) dh and (in|1) (x) dy, NT per thread
    Dp, Hq, Hp, Cp = up4(D + 1), up4(H + 1), up4(H), up4(C)
    T1 = (Dp // 4) * (Hp // 4) if H else 0
    T2 = ((Hq if H else Dp) // 4) * (Cp // 4)
    row_b = 4 * (Dp + (Hq + Hp if H else 0) + Cp) + 12
    p = dict(K=K, Dp=Dp, Hq=Hq, Hp=Hp, Cp=Cp, T1=T1, T2=T2, blocks=T1 + T2,
             NT=((T1 if layer1 else 0) + T2 + THREADS - 1) // THREADS, bwd_row=row_b, bwd_TR=min(BWD_ROWS, LDS // row_b),
             bwd_ok=K <= MAX_K and 16 * (T1 + T2) <= MAX_K)
    # the forward: odd row lengths, the weights in front of the rows when staged
    stage = G == 1 and 4 * K <= W_LDS
    w_floats = up4(K) if stage else 0
    row_f = 4 * ((D | 1) + ((H | 1) if H else 0)) + 12
    TR = min(FWD_ROWS, (LDS - 4 * w_floats) // row_f)
    n_tiles = (rows + TR - 1) // TR
    p.update(stage=stage, w_floats=w_floats, fwd_row=row_f, fwd_TR=TR, n_tiles=n_tiles,
             grid=min(n_tiles, FWD_CAP if stage else FWD_CAP_L2))
    return p


def plan_of(shape, **kw):
    """The plan of a test_gpu_policy_rows.SHAPES row: ((T, N), D, C, H, G, b1, b2, chunk_rows[, blanked tile])."""
    (T, N), D, C, H, G, b1, b2 = shape[:7]
    return plan(D, H, C, G, b1, b2, rows=T * N, **kw)


# (the row, what it is there for: plan values the test asserts).  Rows stay below about 600 so that policy_grad_numpy's
# loop over them stays in seconds; chunk_rows 256 on (2, 63) and on three sets of 63 rows is a single chunk, 7 on 585 rows
# and 5 on 14 leave a short last chunk.  A ninth element blanks that forward tile in a mask (as well as one row).
EDGES = [
    # 256 blocks: NT 1 and every thread owns a block (no thread past the list)
    (((9, 65), 255, 16, 0, 1, False, True, 7), dict(blocks=256, NT=1, K=4096)),
    # 257 blocks: NT 2 with a single block in the second slot; a row of 4,156 B, 15 to a backward tile
    (((2, 63), 1019, 4, 4, 1, True, True, 256), dict(blocks=257, NT=2, bwd_row=4156, bwd_TR=15)),
    # 1,024 blocks (960 + 64), NT 4 with every slot full, behind a hidden layer; one set and three
    (((2, 63), 255, 16, 60, 1, True, True, 7), dict(T1=960, T2=64, NT=4, K=16336, bwd_ok=True)),
    (((3, 63), 255, 16, 60, 3, True, True, 256), dict(T1=960, T2=64, NT=4, K=16336, bwd_ok=True)),
    # K = WG_POLICY_GRAD_MAX_K exactly in 1,024 blocks; three rows to a tile in the backward and, through L2, in the
    # forward; forward tile 2 (rows 6 .. 8 of 14) is blanked
    (((2, 7), 4095, 4, 0, 1, False, True, 5, 2), dict(K=MAX_K, blocks=1024, NT=4, bwd_TR=3, fwd_TR=3, stage=False)),
    # the forward's staging boundary: 32 KiB of weights exactly are staged (7 rows beside them), 8 floats more are not
    (((2, 63), 1024, 8, 0, 1, False, False, 256), dict(K=8192, stage=True, fwd_TR=7)),
    (((2, 63), 1024, 8, 0, 1, False, True, 7), dict(K=8200, stage=False, fwd_TR=15)),
    # staged weights that shrink the tile below 64 rows, with a hidden layer
    (((9, 65), 155, 8, 49, 1, True, True, 256), dict(K=8044, stage=True, fwd_TR=40, NT=3)),
    # the staged layout lw1 | lb1 | lw2 | lb2 with exactly one bias
    (((9, 65), 26, 8, 24, 1, True, False, 7), dict(stage=True, fwd_TR=64)),
    (((9, 65), 26, 8, 24, 1, False, True, 7), dict(stage=True, fwd_TR=64)),
]
AT_LIMIT = [EDGES[2][0], EDGES[4][0]]      # 1,024 blocks with a hidden layer; K at the limit without one
# the second-tile shape of test_forward_walks_more_tiles_than_workgroups: (T, N), D, C, H, G, b1, b2.  199,996 rows are
# 3,125 tiles of 64 with 60 rows in the last (N = 50,000 would fill it)
SECOND_TILE = ((4, 49999), 3, 2, 2, 1, True, True)
