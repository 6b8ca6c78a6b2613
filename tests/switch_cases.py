"""The registry of the package's environment variables: ONE table that the README's switch table, the `os.environ.get("PRD_...")`
calls of protein_redesign_amd/*.py and the GPU tests of the switches are held to (tests/test_switches_cpu.py proves the three sets
equal; tests/test_switches.py parametrises over it).  No device and no library is touched on import.

An entry says how a test sets the switch IN-PROCESS (the variables are read at import, so setting them in os.environ is too late):
  how = "tune"  target = the PRD_TUNE_* bits of include/prd_hip.h       -> lib.prd_set_tune(tune0 | bits), restored in `finally`
  how = "attr"  target = "module.ATTRIBUTE" under protein_redesign_amd   -> monkeypatch.setattr(module, ATTRIBUTE, python value)
  how = "env"   target = the variable itself (read at call time)         -> monkeypatch.setenv(name, value)
  how = "child" the variable selects another library: only a child process can set it (tests/test_ab_build.py)
  how = None    not a switch (`reason` says what it is)
`tests`: "module::function" of the GPU tests that run the non-default arm; every one must exist and carry the gpu mark.
`kind`: "step" = the whole-step test of tests/test_switches.py runs it; "train" = its training test does; "covered" = an older test does.
`split16_only`: the switch cannot change what runs under fp32 arithmetic (the dispatch reads it on a split-16 branch only): the fp32
step must then equal the default arm bit for bit.  `ab_only`: only the -DPRD_AB library carries the selected form; the shipped library
ignores the switch (README) and must give equal bits in BOTH arithmetics.
`trace`: (call of the "# switches" sections of tests/golden/launch_trace.txt.xz, [(b, N, P) of GPU cases that the recording holds]):
the CPU test asserts from the recording that the launches of that call differ between the bit and tune 0.  (The recording's sections
are b = 1 with pair_dim 32 and b = 2 with pair_dim 64 at its own row lengths: the other switches' GPU shapes are not in it.)"""
import collections
import re

Switch = collections.namedtuple("Switch", "value how target attr_value tests kind split16_only ab_only trace reason",
                                defaults=(None, None, None, None, (), None, False, False, None, ""))

T = "test_switches::"
STEP = T + "test_whole_step_under_the_switch"
TRAIN = T + "test_training_switch_off_alone"
AB_FORMS = "test_ab_build::test_superseded_second_generation_forms_in_the_ab_library"
AB_FIRST = "test_ab_build::test_first_generation_kernels_in_the_ab_library"
MERGED = "test_hip_parity::test_fused_launches_equal_their_separate_forms"


def bits(name, tune_defines):
    """the PRD_TUNE_* word of a "tune" entry: a macro name, "TA_VARIANT=<v>" or "TA2_FLAGS=<f>" (the macros with an argument)"""
    m = re.fullmatch(r"(TA_VARIANT|TA2_FLAGS)=(\d+)", name)
    if not m:
        return tune_defines[name]
    if m.group(1) == "TA_VARIANT":
        return int(m.group(2)) & tune_defines["TA_VARIANT_MASK"]
    return tune_defines["TA2_FLAGS_SET"] | ((int(m.group(2)) & 31) << 7)


REGISTRY = {
    # ---- not switches -------------------------------------------------------------------------------------------------------
    "PRD_LIB": Switch(reason="not a switch: the path of the library to load, read once at import (tests/test_ab_build.py loads the A/B build by it)"),
    "PRD_GEMM_MODE": Switch(reason="not a switch: the process default of the arithmetic; every test sets the arithmetic per call (the gemm_mode fixtures)"),
    "PRD_BF16X3": Switch(reason="not a switch: the older spelling of PRD_GEMM_MODE=bf16x3 = split16, the default arithmetic"),
    # ---- PRD_TUNE_* bits: kernel and grid selection inside the library -------------------------------------------------------
    "PRD_TA2_V3": Switch("0", "tune", "TA2_NO_V3", tests=(STEP, T + "test_short_row_core_with_one_barrier_per_phase"), kind="step", split16_only=True,
                         trace=("tri_attn_core_v2", [(1, 33, 32), (1, 384, 32)])),
    "PRD_TA2_LONG": Switch("0", "tune", "TA2_NO_LONG", tests=(STEP, T + "test_long_rows_without_the_second_generation"), kind="step", split16_only=True,
                           trace=("tri_attn", [(1, 385, 32), (1, 417, 32), (1, 449, 32)])),
    "PRD_TA2_XCD8": Switch("0", "tune", "TA2_NO_XCD8", tests=(STEP, T + "test_rows_per_head_not_rounded_to_eight"), kind="step", split16_only=True,
                           trace=("tri_attn", [(1, 449, 32)])),
    "PRD_OL_VARIANT": Switch("1", "tune", "OL_GEN2", tests=(STEP, T + "test_outer_linear_round_two_kernel"), kind="step", split16_only=True),
    "PRD_TMP_NW": Switch("16", "tune", "TMP_NW16", tests=(STEP, T + "test_triangle_multiplication_projection_on_16_waves"), kind="step", split16_only=True),
    "PRD_GEMM_SLAB": Switch("0", "tune", "GEMM_NO_SLAB", tests=(STEP, T + "test_linears_without_the_k_slab_path", T + "test_single_track_without_the_k_slab_path"),
                            kind="step", split16_only=True),
    "PRD_GEMM_KG": Switch("0", "tune", "GEMM_NO_KG", tests=(STEP, T + "test_ring_gemm_one_wave_group"), kind="step", split16_only=True),
    "PRD_GEMM_BRING": Switch("0", "tune", "GEMM_NO_BATCHED_RING", tests=(STEP, T + "test_batched_gemms_on_the_k_split_kernel", T + "test_wide_head_attention_without_the_batched_ring"),
                             kind="step", split16_only=True),
    "PRD_GEMM_XCDCOLS": Switch("1", "tune", "GEMM_XCD_COLS", tests=(STEP, T + "test_tile_gemm_with_the_xcd_column_map"), kind="step", split16_only=True),
    "PRD_TA2_TAIL": Switch("0", "tune", "TA2_NO_TAIL_SPLIT", tests=("test_hip_parity::test_triangle_attention_long_rows_split_tail",), kind="covered"),
    "PRD_TA2_FLAGS": Switch("2", "tune", "TA2_FLAGS=2", tests=("test_hip_parity::test_triangle_attention_long_rows_split_tail",
                                                              "test_hip_parity::test_triangle_attention_long_rows_ragged_key_tail", STEP, AB_FORMS),
                            kind="step", ab_only=True, reason="key-loop forms (bits 1-2) of the short-row core: the step's rows run that core"),
    "PRD_TA2_GV": Switch("0", "tune", "TA2_NO_GV", tests=(STEP, AB_FORMS), kind="step", ab_only=True),
    "PRD_TMS_NW": Switch("16", "tune", "TMS_NW16", tests=("test_hip_parity::test_triangle_multiplication_contraction_direct", STEP, AB_FORMS), kind="step", ab_only=True,
                         reason="12: kept in the shipped library, the second arm of test_triangle_multiplication_contraction_direct; 16: A/B library only"),
    "PRD_TMS_DEPTH": Switch("3", "tune", "TMS_DEPTH3", tests=(STEP, AB_FORMS), kind="step", ab_only=True),
    "PRD_TA_VARIANT": Switch("10", "tune", "TA_VARIANT=10", tests=(STEP, AB_FIRST), kind="step", ab_only=True),
    # ---- host-side switches: module attributes read from the environment at import ------------------------------------------------
    "PRD_HEAD_SLAB": Switch("1", "attr", "trunk._HEAD_SLAB", True, tests=(STEP, T + "test_trunk_head_projection_on_the_k_slab_kernel"), kind="step", split16_only=True),
    "PRD_TRI_MUL_CHAIN": Switch("0", "attr", "trunk._TRI_MUL_CHAIN", False, tests=(STEP, "test_hip_parity::test_triangle_multiplication_chain"), kind="step", split16_only=True),
    "PRD_SPA_CORE": Switch("0", "attr", "ops.SPA_CORE", False, tests=(STEP, T + "test_wide_head_attention_without_the_batched_ring"), kind="step", split16_only=True),
    "PRD_TRI_ATTN_FUSE": Switch("1", "attr", "trunk._TRI_ATTN_FUSE", True, tests=(AB_FIRST,), kind="covered",
                                reason="needs the fused first-generation core of the A/B library: test_triangle_attention_core_with_fused_previous_update runs there"),
    "PRD_PERSISTENT_ATTN": Switch("1", "attr", "ops.PERSISTENT_ATTN", True, tests=("test_hip_parity::test_folding_block_with_the_persistent_attention_pair",), kind="covered"),
    "PRD_MERGE_PROJ": Switch("0", "attr", "trunk._MERGE_PROJ", False, tests=(MERGED,), kind="covered"),
    "PRD_MERGE_HEAD": Switch("0", "attr", "trunk._MERGE_HEAD", False, tests=(MERGED,), kind="covered"),
    "PRD_PAIR_HEAD": Switch("0", "attr", "trunk._PAIR_HEAD", False, tests=(MERGED,), kind="covered"),
    "PRD_FOLD_OUT_PROJ": Switch("0", "attr", "trunk._FOLD_OUT_PROJ", False, tests=("test_single_chain_folded::test_folded_chain_within_2x_of_separate_launches",), kind="covered"),
    # ---- read at call time ----------------------------------------------------------------------------------------------------------
    "PRD_TASK_QUEUE": Switch("1", "env", "PRD_TASK_QUEUE", tests=(STEP, "test_hip_parity::test_block_tail_fusion_and_queue_reset"), kind="step"),
    "PRD_SIDE_STREAM": Switch("1", "env", "PRD_SIDE_STREAM", tests=(STEP, T + "test_side_stream_inside_the_captured_graph"), kind="step"),
    "PRD_FUSED_BOUNDARY": Switch("0", "env", "PRD_FUSED_BOUNDARY", tests=("test_model_widths::test_unfused_boundary_equals_fused",), kind="covered"),
    # ---- training ---------------------------------------------------------------------------------------------------------------------
    "PRD_LIBRARY_BWD": Switch("0", "attr", "training.LIBRARY_BWD", False, tests=(TRAIN,), kind="train"),
    "PRD_HEADS_BWD": Switch("0", "attr", "training.HEADS_BWD", False, tests=(TRAIN,), kind="train"),
    "PRD_INPUT_STAGE_BWD": Switch("0", "attr", "training.INPUT_STAGE_BWD", False, tests=(TRAIN,), kind="train"),
    "PRD_PAIR_LINEAR": Switch("0", "attr", "ops.PAIR_LINEAR", False, tests=(TRAIN,), kind="train"),
    "PRD_TRI_ATTN_BWD_V2": Switch("0", "attr", "ops.TRI_ATTN_BWD_V2", False, tests=(TRAIN,), kind="train"),
    "PRD_TRAIN_FUSED_RESIDUAL": Switch("0", "attr", "training.FUSED_RESIDUAL", False, tests=(TRAIN,), kind="train"),
    "PRD_PAIR_BIAS_BWD": Switch("0", "attr", "training.PAIR_BIAS_BWD", False, tests=("test_training_gpu::test_attention_bias_backward_in_one_pass",), kind="covered"),
    "PRD_TRAIN_CHECKPOINT": Switch("1", "attr", "training.USE_CHECKPOINT", True, tests=("test_head_layouts_backward::test_training_step_gradients_vs_oracle",
                                                                                        "test_nonfinite_guard::test_model_pinned_to_fp32_runs_its_backward_in_fp32"), kind="covered"),
}

# the other key-loop flag forms of the short-row core, as further arms of the whole-step test (same entry: PRD_TA2_FLAGS)
EXTRA_STEP_ARMS = {"PRD_TA2_FLAGS=4": ("PRD_TA2_FLAGS", "TA2_FLAGS=4"), "PRD_TA2_FLAGS=6": ("PRD_TA2_FLAGS", "TA2_FLAGS=6")}


def arms(kind):
    """[(id "PRD_X=v", environment variable, Switch)] of the entries of one kind, in the table's order"""
    out = [(f"{name}={s.value}", name, s) for name, s in REGISTRY.items() if s.kind == kind]
    if kind == "step":
        out += [(aid, name, REGISTRY[name]._replace(value=aid.split("=")[1], target=target)) for aid, (name, target) in EXTRA_STEP_ARMS.items()]
    return out
