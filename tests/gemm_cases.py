"""The case table of the GEMM family (csrc/prd_gemm.hip): ONE list that the CPU dispatch test (tests/test_gemm_dispatch_cpu.py: which
kernel a shape lands on, through the trace driver tests/native/gemm_dispatch_trace.c) and the GPU test (tests/test_gemm_edges.py: that
kernel against float64, inside guarded buffers) are both parametrised over.  No torch, no device and no library is touched on import.

A case states
  id, entry        entry = "gemm" | "ln_rows" | "softmax_rows" | "fc1_folded" | the host queries "slab_ok" | "fc1_folded_ok"
  arith            "fp32" | "split16": the arithmetic the call is made in
  M, N, K, G1, G2  (ln_rows: M = rows, N = C; softmax_rows: M = rows, N = n; fc1_folded: N = Hd, K = S, HC = 64)
  lda, ldb, ldc    leading dimensions, 0 = dense (ln_rows: lda = ldx, ldc = ldy; softmax_rows: ldc = ld)
  a_off, b_off, c_off   element offsets of the operands inside their buffers; spad: extra elements between two batches
  b_kn, a_ln, slab, tile_hint     the flags that bear on dispatch (slab: the call is made with a workspace)
  epi              the epilogue fields in use (names below); opts: their parameters and whatever else the entry takes
  kernels          the kernel name(s) the call must launch, as the launch trace prints them, in launch order; () = a refusal
  ret              the return code (0, or the PRD_ERR_* of a refusal, made before any launch)
  pair             the threshold this case stands beside: the cases of one pair must land on different outcomes
  gpu              False: dispatch only (a refusal, or a shape too large for a quick GPU test)

Epilogue field names: alpha colscale bias addmat colmask act1 act2 act_from rowmask rowmask_cols mulmat mul_pos resid rscale c2 ln_out
out_ln a_scale a_amax.  act_from / rowmask_cols / n_split sit OFF a tile edge (act_from(), rowmask_cols(), n_split() below)."""
import collections

Case = collections.namedtuple("Case", "id entry arith M N K G1 G2 lda ldb ldc a_off b_off c_off spad b_kn a_ln slab tile_hint epi kernels ret pair gpu opts",
                              defaults=(1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, (), (), 0, None, True, None))

ERR_ARG, ERR_ALIGN, ERR_UNSUPPORTED = -1, -2, -3

# ---- kernel names as the trace prints them ------------------------------------------------------------------------------------------
TILE32, TILE64 = "gemm_kernel<32, 32>", "gemm_kernel<64, 64>"          # workgroup tiles of 64 x 64 and 128 x 128
SKINNY4, SKINNY4_LN, SKINNY8 = "gemm_skinny_kernel<4, false>", "gemm_skinny_kernel<4, true>", "gemm_skinny_kernel<8, false>"
H2_1, H2_4 = "gemm_h2_kernel<1>", "gemm_h2_kernel<4>"
SLAB, SLAB_X, SLAB_REDUCE, FOLD_REDUCE = "gemm_slab_kernel<0>", "gemm_slab_kernel<1>", "gemm_slab_reduce_kernel", "fc1_fold_reduce_kernel<64>"
LN_ROWS, LN_ROWS64, SOFTMAX = "ln_rows_kernel", "ln_rows64_kernel", "softmax_rows_kernel"
RING_BKN = "gemm_ring_kernel<8, 1, false, true>"


def ring(D, KG, ln=False):
    return f"gemm_ring_kernel<{D}, {KG}, {'true' if ln else 'false'}, false>"


# instantiated by the two-way LayerNorm dispatch of launch_ring, never launched (tests/test_launch_trace_cpu.py: NOT_TRACED)
NEVER_LAUNCHED = {ring(4, 4, True)}

E0 = ("bias", "act1", "resid")                                          # the epilogue of the shape cases: no zero row, no zero column
# every field a tile / skinny / h2 / ring kernel accepts, in two cases: the first with the restricted / scaled forms ...
EPI_A = ("alpha", "colscale", "bias", "addmat", "act1", "act_from", "rowmask", "rowmask_cols", "mulmat", "resid", "rscale", "c2")
# ... the second with the plain ones, the column mask and the sign mask
EPI_B = ("bias", "colmask", "act2", "act_from", "rowmask", "mulmat", "mul_pos", "resid")
# what prd_gemm lets through to the K-slab path
EPI_S = ("alpha", "colscale", "bias", "act1", "act_from", "rowmask", "rowmask_cols", "resid", "rscale", "c2")


def _odd_off_edge(v):
    v |= 1
    return v + 2 if v % 32 in (1, 31) else v                            # odd, and not next to a multiple of 32 either


def act_from(c):
    return (c.opts or {}).get("act_from", _odd_off_edge(c.N // 2)) if "act_from" in c.epi else 0


def rowmask_cols(c):
    return (c.opts or {}).get("rowmask_cols", _odd_off_edge(c.N // 3)) if "rowmask_cols" in c.epi else 0


def n_split(c):
    """columns n >= n_split go to C2: off a tile edge; a multiple of 4 (and of no 32) where the case asks for the K-slab path"""
    if "c2" not in c.epi:
        return 0
    if "n_split" in (c.opts or {}):
        return c.opts["n_split"]
    if c.slab:
        v = (5 * c.N // 8) // 4 * 4
        return v + 4 if v % 32 == 0 else v
    return _odd_off_edge(5 * c.N // 8)


CASES = []


def add(id, entry, arith, M, N, K, kernels, **kw):
    assert all(c.id != id for c in CASES), id
    CASES.append(Case(id, entry, arith, M, N, K, kernels=tuple(kernels), **kw))


def gemm(id, arith, M, N, K, kernels, epi=E0, **kw):
    add(id, "gemm", arith, M, N, K, kernels, epi=epi, **kw)


def slab(id, M, N, K, nslab, spw, xmap, epi=E0, **kw):
    """a call the K-slab path takes: both launches, and the split the first one must be given"""
    opts = dict(kw.pop("opts", None) or {}, nslab=nslab, spw=spw, xmap=xmap)
    gemm(id, "split16", M, N, K, (SLAB, SLAB_REDUCE), epi=epi, slab=1, opts=opts, **kw)


S16, F32 = "split16", "fp32"
ADDR = dict(a_off=4, b_off=8, c_off=12, spad=20)                        # offsets that are multiples of 4, batch strides that are not the dense ones

# ---- operand ring (split-16, fewer than 512 tiles of 64 x 64, K % 64 == 0): nine (D, KG) forms by chunk count and tile count ----------
gemm("ring_k512_t64", S16, 256, 256, 512, [ring(2, 4)], pair="ring k512: 64 | 65 tiles of 32 x 32")
gemm("ring_k512_t72", S16, 257, 256, 512, [ring(4, 2)], pair="ring k512: 64 | 65 tiles of 32 x 32")
gemm("ring_k512_t192", S16, 384, 512, 512, [ring(4, 2)], pair="ring k512: 192 | 193 tiles of 32 x 32")
gemm("ring_k512_t208", S16, 385, 512, 512, [ring(8, 1)], pair="ring k512: 192 | 193 tiles of 32 x 32")
gemm("ring_k256_t128", S16, 256, 512, 256, [ring(2, 2)], pair="ring k256: 128 | 129 tiles of 32 x 32")
gemm("ring_k256_t144", S16, 257, 512, 256, [ring(4, 1)], pair="ring k256: 128 | 129 tiles of 32 x 32")
gemm("ring_k64", S16, 77, 33, 64, [ring(1, 1)], pair="ring chunks 1 | 2")
gemm("ring_k128", S16, 77, 33, 128, [ring(2, 1)], pair="ring chunks 1 | 2")
gemm("ring_k128_b", S16, 90, 40, 128, [ring(2, 1)], pair="ring chunks 2 | 3")
gemm("ring_k192", S16, 90, 40, 192, [ring(4, 1)], pair="ring chunks 2 | 3")
gemm("ring_k256_many", S16, 257, 544, 256, [ring(4, 1)], pair="ring chunks 4 | 5")
gemm("ring_k320", S16, 257, 544, 320, [ring(8, 1)], pair="ring chunks 4 | 5")
gemm("ring_k448", S16, 77, 33, 448, [ring(8, 1)])
gemm("ring_k512_one_group", S16, 385, 544, 512, [ring(8, 1)], pair="ring chunks 8 | 9")
gemm("ring_k576", S16, 385, 544, 576, [ring(8, 2)], pair="ring chunks 8 | 9")
gemm("ring_k1024", S16, 50, 96, 1024, [ring(8, 2)], pair="ring chunks 16 | 17")
gemm("ring_k1088", S16, 50, 96, 1088, [ring(4, 4)], pair="ring chunks 16 | 17")
gemm("ring_k576_t1024", S16, 1024, 1024, 576, [ring(8, 2)], pair="ring beyond 8 chunks: 1024 | 1025 tiles of 32 x 32")
gemm("ring_k576_many", S16, 1056, 1056, 576, [ring(4, 1)], pair="ring beyond 8 chunks: 1024 | 1025 tiles of 32 x 32")
# with the fused LayerNorm of the A rows: the same forms, <4, 4> excepted
gemm("ring_ln_k64", S16, 77, 33, 64, [ring(1, 1, True)], a_ln=1, epi=("bias", "ln_out"))
gemm("ring_ln_k128", S16, 77, 33, 128, [ring(2, 1, True)], a_ln=1, epi=("bias", "act1"))
gemm("ring_ln_k192", S16, 90, 40, 192, [ring(4, 1, True)], a_ln=1, epi=("bias", "ln_out"))
gemm("ring_ln_k320", S16, 65, 70, 320, [ring(8, 1, True)], a_ln=1, epi=("bias", "act1", "ln_out"))
gemm("ring_ln_k256_t128", S16, 256, 512, 256, [ring(2, 2, True)], a_ln=1, epi=("bias", "ln_out"))
gemm("ring_ln_k512_t64", S16, 256, 256, 512, [ring(2, 4, True)], a_ln=1, epi=("bias", "act1", "ln_out"))
gemm("ring_ln_k512_t72", S16, 257, 256, 512, [ring(4, 2, True)], a_ln=1, epi=("bias", "ln_out"))
gemm("ring_ln_k1024", S16, 50, 96, 1024, [ring(8, 2, True)], a_ln=1, epi=("bias", "ln_out"), pair="a_ln: K 1024 | 1088")
gemm("ring_ln_k1088_refused", S16, 50, 96, 1088, [], a_ln=1, epi=("bias",), ret=ERR_UNSUPPORTED, gpu=False, pair="a_ln: K 1024 | 1088")
# batched, and B as [K][N]
gemm("ring_batched", S16, 45, 70, 128, [ring(2, 1)], G1=2, G2=3, pair="batched ring: without | with a_ln", **ADDR, lda=132, ldb=136, ldc=72)
gemm("ring_batched_ln_skinny", S16, 45, 70, 128, [SKINNY4_LN], G1=2, G2=3, a_ln=1, epi=("bias", "act1"), pair="batched ring: without | with a_ln")
gemm("bkn_k64", S16, 45, 70, 64, [RING_BKN], G1=2, G2=2, b_kn=1, epi=("bias", "mulmat"), **ADDR, lda=68, ldb=76, ldc=72)
gemm("bkn_k512", S16, 320, 96, 512, [RING_BKN], G1=1, G2=2, b_kn=1, epi=("mulmat",), pair="[K][N] ring: K 512 | 576")
gemm("bkn_k576_skinny", S16, 320, 96, 576, [SKINNY4], G1=1, G2=2, b_kn=1, epi=("mulmat",), pair="[K][N] ring: K 512 | 576")
gemm("bkn_n4", S16, 33, 4, 128, [RING_BKN], b_kn=1, epi=("bias",), pair="[K][N] ring: N 3 | 4")
gemm("bkn_n3_skinny", S16, 33, 3, 128, [SKINNY4], b_kn=1, ldb=4, epi=("bias",), pair="[K][N] ring: N 3 | 4")
gemm("bkn_softmax", S16, 70, 48, 192, [RING_BKN], G1=2, G2=2, b_kn=1, a_ln=2, epi=("mulmat", "a_scale"), pair="a_ln = 2: [K][N] ring | elsewhere")
gemm("softmax_a_refused", S16, 70, 48, 192, [], a_ln=2, epi=(), ret=ERR_UNSUPPORTED, gpu=False, pair="a_ln = 2: [K][N] ring | elsewhere")
gemm("bkn_softmax_k576_refused", S16, 70, 48, 576, [], b_kn=1, a_ln=2, epi=(), ret=ERR_UNSUPPORTED, gpu=False)

# ---- split-16 tile kernel (at least 512 tiles of 64 x 64, K % 32 == 0) ------------------------------------------------------------------
gemm("h2_t512", S16, 1024, 2048, 512, [H2_1], pair="64 x 64 tiles 511 | 512")
gemm("ring_t480", S16, 960, 2048, 512, [ring(8, 1)], pair="64 x 64 tiles 511 | 512")
gemm("h2_k992", S16, 1024, 2048, 992, [H2_1], pair="h2: K 992 | 1024")
gemm("h2_k1024", S16, 1024, 2048, 1024, [H2_4], pair="h2: K 992 | 1024")
gemm("h2_k96", S16, 1024, 2048, 96, [H2_1], pair="split-16, 512 tiles: K % 32 == 0 | not")
gemm("tile_k100_split16", S16, 1024, 2048, 100, [TILE32], pair="split-16, 512 tiles: K % 32 == 0 | not")
gemm("skinny_k96_split16", S16, 77, 33, 96, [SKINNY4], pair="split-16, few tiles: K % 64 == 0 | not")
gemm("ring_k128_c", S16, 77, 33, 128, [ring(2, 1)], epi=("bias",), pair="split-16, few tiles: K % 64 == 0 | not")
gemm("h2_ln", S16, 1024, 2048, 512, [H2_1], a_ln=1, epi=("bias", "act1", "ln_out"))
gemm("h2_k1024_ln", S16, 1023, 2049, 1024, [H2_4], a_ln=1, epi=("bias", "ln_out"))

# ---- fp32: K-split kernel below 512 tiles of 64 x 64, tile kernels from there ------------------------------------------------------
gemm("skinny4", F32, 320, 2048, 512, [SKINNY4])
gemm("skinny8_k1024", F32, 50, 96, 1024, [SKINNY8], pair="fp32 skinny: K 1020 | 1024")
gemm("skinny4_k1020", F32, 50, 96, 1020, [SKINNY4], pair="fp32 skinny: K 1020 | 1024")
gemm("skinny8_t512", F32, 512, 1024, 1024, [SKINNY8], pair="fp32 skinny, K 1024: 512 | 513 tiles of 32 x 32")
gemm("skinny4_t544", F32, 513, 1024, 1024, [SKINNY4], pair="fp32 skinny, K 1024: 512 | 513 tiles of 32 x 32")
gemm("tile32_t512", F32, 1024, 2048, 36, [TILE32], pair="fp32: 64 x 64 tiles 511 | 512")
gemm("skinny4_t480", F32, 960, 2048, 36, [SKINNY4], pair="fp32: 64 x 64 tiles 511 | 512")
gemm("tile32_t1024", F32, 2048, 2048, 36, [TILE32], pair="fp32: 64 x 64 tiles 1024 | 1025")
gemm("tile64_t1089", F32, 2112, 2112, 36, [TILE64], pair="fp32: 64 x 64 tiles 1024 | 1025")
gemm("tile32_m64", F32, 64, 65600, 36, [TILE32], pair="fp32, more than 1024 tiles: M 64 | 65")
gemm("tile64_m65", F32, 65, 65600, 36, [TILE64], pair="fp32, more than 1024 tiles: M 64 | 65")
gemm("skinny_ln", F32, 70, 21, 512, [SKINNY4_LN], a_ln=1, epi=("bias", "act1", "ln_out"), pair="fp32 a_ln: K 512 | 516")
gemm("skinny_ln_k516_refused", F32, 70, 21, 516, [], a_ln=1, epi=("bias",), ret=ERR_UNSUPPORTED, gpu=False, pair="fp32 a_ln: K 512 | 516")
gemm("skinny_ln_k36", F32, 33, 31, 36, [SKINNY4_LN], a_ln=1, epi=("bias", "ln_out"))
gemm("skinny_bkn", F32, 45, 16, 45, [SKINNY4], G1=2, G2=4, b_kn=1, lda=48, epi=("mulmat",))
gemm("tile32_bkn", F32, 45, 16, 45, [TILE32], G1=2, G2=4, b_kn=1, lda=48, tile_hint=64, epi=("mulmat",))

# ---- the K-slab path (split-16, a workspace, M >= 96, K % 128 == 0, N % 4 == 0, tiles x slabs >= 128) ------------------------------------
slab("slab_m96", 96, 2048, 512, 4, 1, 2, pair="slab: M 95 | 96")
gemm("slab_m95_ring", S16, 95, 2048, 512, [ring(4, 2)], slab=1, pair="slab: M 95 | 96")
slab("slab_work128_sk1", 160, 8192, 128, 1, 1, 2, pair="slab: tiles x slabs 127 | 128")
gemm("slab_work127_ring", S16, 160, 8128, 128, [ring(2, 1)], slab=1, pair="slab: tiles x slabs 127 | 128")
slab("slab_sk1_odd", 160, 8256, 128, 1, 1, 0, pair="slab map, one slab group: tiles_n % 8 == 0 | not")
slab("slab_sk1_even", 160, 8704, 128, 1, 1, 2, pair="slab map, one slab group: tiles_n % 8 == 0 | not")
slab("slab_sk2_odd", 480, 1472, 256, 2, 1, 0, pair="slab map, two slab groups: tiles_n % 4 == 0 | not")
slab("slab_sk2_even", 480, 1536, 256, 2, 1, 2, pair="slab map, two slab groups: tiles_n % 4 == 0 | not")
slab("slab_sk3", 320, 1408, 384, 3, 1, 0)
slab("slab_sk5", 320, 832, 640, 5, 1, 0)
slab("slab_sk7", 320, 640, 896, 7, 1, 0, pair="slab map: 7 | 8 slab groups")
slab("slab_sk8", 320, 640, 1024, 8, 1, 1, pair="slab map: 7 | 8 slab groups")
slab("slab_sk9", 100, 960, 1152, 9, 1, 0)
slab("slab_ragged_group", 2560, 512, 1280, 10, 3, 2)                      # slab groups of 3, 3, 3 and 1
slab("slab_spw1", 320, 2048, 1024, 8, 1, 1, pair="slab: tiles x slabs 512 | 528, one | two slabs per workgroup")
slab("slab_spw2", 320, 2112, 1024, 8, 2, 0, pair="slab: tiles x slabs 512 | 528, one | two slabs per workgroup")
slab("slab_n2048", 320, 2048, 512, 4, 1, 2, pair="slab: N % 4 == 0 | not")
gemm("slab_n2046_ring", S16, 320, 2046, 512, [ring(8, 1)], slab=1, pair="slab: N % 4 == 0 | not")
slab("slab_k512", 320, 1028, 512, 4, 1, 0, pair="slab: K % 128 == 0 | not")
gemm("slab_k576_ring", S16, 320, 1028, 576, [ring(8, 2)], slab=1, pair="slab: K % 128 == 0 | not")
slab("slab_tiles4096", 10240, 4096, 128, 1, 1, 2, gpu=False, pair="slab: 4096 | 4097 tiles")
gemm("slab_tiles4160_h2", S16, 10400, 4096, 128, [H2_1], slab=1, gpu=False, pair="slab: 4096 | 4097 tiles")
gemm("slab_fp32_skinny", F32, 320, 2048, 512, [SKINNY4], slab=1, pair="slab: split-16 | fp32")
slab("slab_split16", 320, 2048, 512, 4, 1, 2, epi=("bias",), pair="slab: split-16 | fp32")
gemm("slab_hint_skinny", S16, 320, 2048, 512, [SKINNY4], slab=1, tile_hint=32)

# ---- ragged tiles on every family: M, N one below, at and one above the family's tile; M = 1; N = 5 (4 where b_kn needs it) -------------
for m, n in ((31, 33), (32, 32), (33, 31), (1, 5)):
    gemm(f"ring_{m}x{n}", S16, m, n, 128, [ring(2, 1)])
    gemm(f"ring_ln_{m}x{n}", S16, m, n, 256, [ring(2, 2, True)], a_ln=1, epi=("bias", "ln_out"))
    gemm(f"bkn_{m}x{n + (-n) % 4}", S16, m, n + (-n) % 4, 128, [RING_BKN], b_kn=1)
    for k in (1, 3, 36):
        gemm(f"skinny_{m}x{n}_k{k}", F32, m, n, k, [SKINNY4], lda=4 * ((k + 3) // 4), ldb=4 * ((k + 3) // 4))
    gemm(f"skinny8_{m}x{n}", F32, m, n, 1028, [SKINNY8])
for m, n in ((63, 65), (64, 64), (65, 63), (1, 5)):
    for k in (1, 3, 36):
        gemm(f"tile32_{m}x{n}_k{k}", F32, m, n, k, [TILE32], tile_hint=64, lda=4 * ((k + 3) // 4), ldb=4 * ((k + 3) // 4))
for m, n in ((127, 129), (128, 128), (129, 127), (1, 5)):
    for k in (1, 3, 36):
        gemm(f"tile64_{m}x{n}_k{k}", F32, m, n, k, [TILE64], tile_hint=128, lda=4 * ((k + 3) // 4), ldb=4 * ((k + 3) // 4))
gemm("h2_1023x2049", S16, 1023, 2049, 64, [H2_1])
gemm("h2_1025x2047", S16, 1025, 2047, 64, [H2_1])
gemm("h2_k1024_1023x2049", S16, 1023, 2049, 1056, [H2_4])
gemm("h2_m1", S16, 1, 32773, 64, [H2_1])
gemm("h2_n5", S16, 32773, 5, 64, [H2_1])
slab("slab_159x1020", 159, 1020, 1024, 8, 1, 1)
slab("slab_160x1024", 160, 1024, 1024, 8, 1, 1)
slab("slab_161x1028", 161, 1028, 1024, 8, 1, 1)

# ---- addressing: lda > K, ldb > K, ldc > N, offsets that are multiples of 4, batch strides that are not the dense ones ------------------
gemm("addr_tile32", F32, 70, 75, 36, [TILE32], G1=2, G2=3, tile_hint=64, lda=40, ldb=44, ldc=80, **ADDR)
gemm("addr_tile64", F32, 130, 75, 36, [TILE64], G1=3, G2=1, tile_hint=128, lda=40, ldb=44, ldc=80, **ADDR)
gemm("addr_skinny4", F32, 70, 75, 200, [SKINNY4], G1=2, G2=3, lda=204, ldb=208, ldc=80, **ADDR)
gemm("addr_skinny8", F32, 70, 75, 1100, [SKINNY8], G1=1, G2=2, lda=1104, ldb=1108, ldc=80, **ADDR)
gemm("addr_skinny_ln", F32, 70, 75, 200, [SKINNY4_LN], G1=2, G2=1, a_ln=1, epi=("bias",), lda=204, ldb=208, ldc=80, **ADDR)
gemm("addr_ring", S16, 70, 75, 320, [ring(8, 1)], G1=2, G2=2, lda=324, ldb=328, ldc=80, **ADDR)
gemm("addr_ring_ln", S16, 70, 75, 320, [ring(8, 1, True)], a_ln=1, epi=("bias", "ln_out"), lda=324, ldb=328, ldc=80, **ADDR)
gemm("addr_h2", S16, 1024, 2045, 64, [H2_1], lda=68, ldb=72, ldc=2052, **ADDR)
slab("addr_slab", 320, 1028, 512, 4, 1, 0, lda=516, ldb=520, ldc=1036, **ADDR)

# ---- the epilogue, field by field, at indices off a tile edge ----------------------------------------------------------------------
for name, arith, m, n, k, kern, kw in (("tile32", F32, 70, 150, 36, TILE32, dict(tile_hint=64)), ("tile64", F32, 140, 150, 36, TILE64, dict(tile_hint=128)),
                                       ("skinny4", F32, 70, 150, 100, SKINNY4, {}), ("skinny8", F32, 70, 150, 1024, SKINNY8, {}),
                                       ("h2", S16, 1024, 2047, 64, H2_1, {}), ("h2_kg4", S16, 1024, 2047, 1024, H2_4, {}),
                                       ("ring", S16, 70, 150, 320, ring(8, 1), {}), ("ring_kg", S16, 70, 150, 512, ring(2, 4), {}),
                                       ("bkn", S16, 70, 152, 128, RING_BKN, dict(b_kn=1))):
    gemm(f"epi_a_{name}", arith, m, n, k, [kern], epi=EPI_A, **kw)
    gemm(f"epi_b_{name}", arith, m, n, k, [kern], epi=EPI_B, **kw)
gemm("epi_b_tile32_batched", F32, 70, 150, 36, [TILE32], G1=2, G2=2, tile_hint=64, epi=EPI_B)     # colmask [G1][N], rowmask [G1][M]
gemm("epi_b_ring_batched", S16, 70, 150, 128, [ring(2, 1)], G1=2, G2=2, epi=EPI_B)
gemm("epi_b_skinny_ln", F32, 70, 150, 100, [SKINNY4_LN], a_ln=1, epi=EPI_B + ("ln_out",))
gemm("epi_a_ring_ln", S16, 70, 150, 320, [ring(8, 1, True)], a_ln=1, epi=EPI_A + ("ln_out",))
gemm("epi_ring_a_scale", S16, 70, 150, 320, [ring(8, 1)], epi=("alpha", "a_scale", "mulmat"))
gemm("epi_h2_a_amax", S16, 1024, 2047, 64, [H2_1], epi=("alpha", "a_amax"))
gemm("epi_h2_kg4_a_amax", S16, 1024, 2047, 1024, [H2_4], epi=("alpha", "a_amax"))
# the reduce launch of the K-slab path applies the epilogue in code of its own: every field prd_gemm lets through ...
slab("epi_slab", 320, 1028, 512, 4, 1, 0, epi=EPI_S)
slab("epi_slab_wide", 173, 1284, 1024, 8, 1, 1, epi=("bias", "act2", "act_from", "rowmask", "resid", "c2"))
slab("epi_slab_ln", 320, 2048, 512, 4, 1, 2, a_ln=1, epi=("bias", "act1", "ln_out"))
slab("epi_slab_ln_c2", 161, 1028, 512, 4, 1, 0, a_ln=1, epi=("alpha", "colscale", "bias", "act2", "act_from", "rowmask", "rowmask_cols", "resid", "rscale", "c2", "ln_out"))
slab("epi_slab_out_ln", 320, 512, 2048, 16, 1, 1, epi=("bias", "resid", "out_ln"), pair="out_ln: N 512 | 516")
gemm("epi_slab_out_ln_n516_refused", S16, 320, 516, 2048, [], slab=1, epi=("bias", "resid", "out_ln"), ret=ERR_UNSUPPORTED, gpu=False, pair="out_ln: N 512 | 516")
slab("epi_slab_out_ln_ragged", 333, 340, 1024, 8, 1, 1, epi=("alpha", "bias", "act1", "act_from", "resid", "rscale", "out_ln"))
# ... and one case per field it does not: the call lands on the ring kernel and is still right
gemm("epi_slab_addmat_ring", S16, 320, 1028, 512, [ring(8, 1)], slab=1, epi=("bias", "addmat"), pair="slab: without | with addmat")
slab("epi_slab_bias", 320, 1028, 512, 4, 1, 0, epi=("bias",), pair="slab: without | with addmat")
gemm("epi_slab_colmask_ring", S16, 320, 1028, 512, [ring(8, 1)], slab=1, epi=("bias", "colmask"))
gemm("epi_slab_mulmat_ring", S16, 320, 1028, 512, [ring(8, 1)], slab=1, epi=("bias", "mulmat"))
gemm("epi_slab_c2_odd_ring", S16, 320, 1028, 512, [ring(8, 1)], slab=1, epi=("bias", "c2"), opts=dict(n_split=643), pair="slab: n_split % 4 == 0 | not")
slab("epi_slab_c2", 320, 1028, 512, 4, 1, 0, epi=("bias", "c2"), opts=dict(n_split=644), pair="slab: n_split % 4 == 0 | not")
gemm("epi_slab_ln_no_wsum_ring", S16, 320, 1028, 512, [ring(8, 1, True)], slab=1, a_ln=1, epi=("bias",), opts=dict(no_wsum=1))

# ---- refusals, before any launch ------------------------------------------------------------------------------------------------------
gemm("refuse_out_ln_no_ws", S16, 320, 512, 2048, [], epi=("bias", "out_ln"), ret=ERR_UNSUPPORTED, gpu=False)
gemm("refuse_out_ln_fp32", F32, 320, 512, 2048, [], slab=1, epi=("bias", "out_ln"), ret=ERR_UNSUPPORTED, gpu=False)
gemm("refuse_lda", S16, 77, 33, 64, [], lda=66, ret=ERR_ALIGN, gpu=False)
gemm("refuse_ldb", F32, 77, 33, 36, [], lda=36, ldb=38, ret=ERR_ALIGN, gpu=False)
gemm("refuse_ln_out_without_a_ln", S16, 77, 33, 64, [], epi=("ln_out",), ret=ERR_ARG, gpu=False)
gemm("refuse_c2_batched", S16, 77, 33, 64, [], G1=2, epi=("c2",), ret=ERR_ARG, gpu=False)
gemm("refuse_a_ln_bkn", F32, 77, 36, 64, [], a_ln=1, b_kn=1, ret=ERR_UNSUPPORTED, gpu=False)
gemm("refuse_a_ln_hint64", F32, 77, 33, 64, [], a_ln=1, tile_hint=64, ret=ERR_UNSUPPORTED, gpu=False)

# ---- prd_single_fc1_folded: the K-slab GEMM on [single | og] with the second A segment, and its own reduce launch -----------------------
for m, ok in ((95, 0), (96, 1), (333, 1), (640, 1), (641, 0)):
    add(f"fc1_m{m}", "fc1_folded", S16, m, 2048, 512, [SLAB_X, FOLD_REDUCE] if ok else [], ret=0 if ok else ERR_UNSUPPORTED, gpu=bool(ok),
        opts=dict(nslab=4, spw=1, xmap=2), pair={95: "fc1 folded: M 95 | 96", 96: "fc1 folded: M 95 | 96", 640: "fc1 folded: M 640 | 641", 641: "fc1 folded: M 640 | 641"}.get(m))
    add(f"fc1_ok_m{m}", "fc1_folded_ok", S16, m, 2048, 512, [], ret=ok, gpu=False)
add("fc1_fp32_refused", "fc1_folded", F32, 320, 2048, 512, [], ret=ERR_UNSUPPORTED, gpu=False)
add("fc1_ok_s256", "fc1_folded_ok", S16, 320, 1024, 256, [], ret=0, gpu=False)                     # two slab groups: not the tested form
for (m, n, k), ok in (((96, 2048, 512), 1), ((95, 2048, 512), 0), ((160, 8192, 128), 1), ((160, 8128, 128), 0), ((320, 2046, 512), 0), ((320, 2048, 576), 0),
                      ((10240, 4096, 128), 1), ((10400, 4096, 128), 0)):
    add(f"slab_ok_{m}x{n}x{k}", "slab_ok", S16, m, n, k, [], ret=ok, gpu=False)
add("slab_ok_fp32", "slab_ok", F32, 320, 2048, 512, [], ret=0, gpu=False)

# ---- prd_ln_rows: ln_rows64_kernel at C == 64, 16-byte alignment and rows >= 4096, the wave-per-row kernel elsewhere --------------------
def ln(id, rows, C, kernel, **kw):
    add(id, "ln_rows", F32, rows, C, 0, [kernel], **kw)


ln("ln64_r4095", 4095, 64, LN_ROWS, pair="ln_rows, C 64: rows 4095 | 4096")
ln("ln64_r4096", 4096, 64, LN_ROWS64, pair="ln_rows, C 64: rows 4095 | 4096")
ln("ln64_r4099", 4099, 64, LN_ROWS64, opts=dict(gamma=1))
ln("ln64_r4099_pitched", 4099, 64, LN_ROWS64, lda=68, ldc=72, opts=dict(gamma=1), pair="ln_rows, C 64: ldx % 4 == 0 | not")
ln("ln64_r4099_ldx66", 4099, 64, LN_ROWS, lda=66, ldc=72, opts=dict(gamma=1), pair="ln_rows, C 64: ldx % 4 == 0 | not")
ln("ln64_r4096_aligned", 4096, 64, LN_ROWS64, opts=dict(gamma=1), pair="ln_rows, C 64: x 16-byte aligned | 4 bytes off")
ln("ln64_r4096_x_off4", 4096, 64, LN_ROWS, a_off=1, opts=dict(gamma=1), pair="ln_rows, C 64: x 16-byte aligned | 4 bytes off")
ln("ln63_r4096", 4096, 63, LN_ROWS, pair="ln_rows, 4096 rows: C 63 | 64")
ln("ln64_r4096_b", 4096, 64, LN_ROWS64, lda=64, pair="ln_rows, 4096 rows: C 63 | 64")
ln("ln65_r4096", 4096, 65, LN_ROWS, pair="ln_rows, 4096 rows: C 64 | 65")
ln("ln64_r4096_c", 4096, 64, LN_ROWS64, ldc=64, pair="ln_rows, 4096 rows: C 64 | 65")
for C in (1, 63, 65, 1280):
    for rows in (1, 5):
        for gamma in (0, 1):
            if C > 1 or gamma:                                          # (one channel without affine is all zeros: nothing to measure)
                ln(f"ln{C}_r{rows}_g{gamma}", rows, C, LN_ROWS, opts=dict(gamma=gamma))
ln("ln1280_pitched", 5, 1280, LN_ROWS, lda=1284, ldc=1291, opts=dict(gamma=1))
ln("ln63_pitched", 5, 63, LN_ROWS, lda=67, ldc=64)

# ---- prd_softmax_rows: one wave per row, the tail [n, ld) zero-filled ------------------------------------------------------------------
for n in (1, 63, 64, 65, 141):
    for pad in (0, 3, 67):
        for rows in (1, 5):
            add(f"softmax_n{n}_ld{n + pad}_r{rows}", "softmax_rows", F32, rows, n, 0, [SOFTMAX], ldc=n + pad)
add("softmax_gap200", "softmax_rows", F32, 5, 141, 0, [SOFTMAX], ldc=144, opts=dict(gap=200.0))

BY_ID = {c.id: c for c in CASES}
GPU_CASES = [c for c in CASES if c.gpu]


def pairs():
    """{threshold: [its cases]}"""
    out = collections.OrderedDict()
    for c in CASES:
        if c.pair:
            out.setdefault(c.pair, []).append(c)
    return out


# ---- what the shape implies ----------------------------------------------------------------------------------------------------------
def ceil_div(a, b):
    return (a + b - 1) // b


def dims(c):
    """(lda, ldb, ldc) with the dense defaults filled in"""
    return (c.lda or c.K, c.ldb or (c.N if c.b_kn else c.K), c.ldc or c.N)


def expected_launches(c):
    """[(kernel, grid, block)] of the case: the grid and block that its shape implies for each kernel it names"""
    G, o = c.G1 * c.G2, c.opts or {}
    out = []
    for k in c.kernels:
        if k in (TILE32, TILE64):
            t = 64 if k == TILE32 else 128
            out.append((k, (ceil_div(c.M, t) * ceil_div(c.N, t), G, 1), (256, 1, 1)))
        elif k.startswith("gemm_skinny_kernel"):
            out.append((k, (ceil_div(c.M, 32) * ceil_div(c.N, 32), G, 1), (512 if k == SKINNY8 else 256, 1, 1)))
        elif k.startswith("gemm_h2_kernel"):
            out.append((k, (ceil_div(c.M, 64) * ceil_div(c.N, 64), 1, 1), (1024 if k == H2_4 else 256, 1, 1)))
        elif k.startswith("gemm_ring_kernel"):
            kg = int(k.split(",")[1])
            out.append((k, (ceil_div(c.M, 32) * ceil_div(c.N, 32), G, 1), (256 * kg, 1, 1)))
        elif k in (SLAB, SLAB_X):
            out.append((k, (ceil_div(c.M, 160) * ceil_div(c.N, 64) * ceil_div(o["nslab"], o["spw"]), 1, 1), (640, 1, 1)))
        elif k == SLAB_REDUCE:
            out.append((k, (c.M * ceil_div(c.N, 512), 1, 1), (128, 1, 1)))
        elif k == FOLD_REDUCE:
            out.append((k, (c.M, 1, 1), (128 * ceil_div(c.N, 512), 1, 1)))
        elif k == LN_ROWS64:
            out.append((k, (ceil_div(c.M, 16), 1, 1), (256, 1, 1)))
        elif k in (LN_ROWS, SOFTMAX):
            out.append((k, (ceil_div(c.M, 4), 1, 1), (256, 1, 1)))
        else:
            raise KeyError(k)
    return out


def driver_line(c):
    """the line of tests/native/gemm_dispatch_trace.c for this case"""
    o = c.opts or {}
    kv = dict(arith=1 if c.arith == S16 else 0)
    if c.entry == "gemm":
        lda, ldb, ldc = dims(c)
        kv.update(M=c.M, N=c.N, K=c.K, G1=c.G1, G2=c.G2, lda=lda, ldb=ldb, ldc=ldc, b_kn=c.b_kn, a_ln=c.a_ln, tile_hint=c.tile_hint, ws=c.slab,
                  act=1 if "act1" in c.epi else 2 if "act2" in c.epi else 0, act_from=act_from(c), rowmask_cols=rowmask_cols(c), n_split=n_split(c),
                  mul_pos=int("mul_pos" in c.epi), ldadd=c.N + 4, ldmul=c.N + 8, ldr=c.N + 4, ldlo=c.K + 4, ldol=c.N + 4, ldc2=c.N - n_split(c) + 4,
                  wsum=int(bool(c.slab and c.a_ln and not o.get("no_wsum"))))
        for f in ("colscale", "bias", "addmat", "colmask", "rowmask", "mulmat", "resid", "rscale", "ln_out", "out_ln", "a_amax"):
            kv[f] = int(f in c.epi)
        kv["C2"] = int("c2" in c.epi)
    elif c.entry == "ln_rows":
        kv = dict(rows=c.M, C=c.N, ldx=c.lda or c.N, ldy=c.ldc or c.N, gamma=o.get("gamma", 0), x=2 if c.a_off % 4 else 1)
    elif c.entry == "softmax_rows":
        kv = dict(rows=c.M, n=c.N, ld=c.ldc or c.N)
    elif c.entry in ("fc1_folded", "fc1_folded_ok"):
        kv.update(M=c.M, S=c.K, HC=64, Hd=c.N)
    elif c.entry == "slab_ok":
        kv.update(M=c.M, N=c.N, K=c.K)
    return f"{c.id} {c.entry} " + " ".join(f"{k}={v}" for k, v in kv.items())
