"""The integer codes of csrc/include/svdj_hip.h (tests/test_codes_cpu.py pins
them to it).  Plain integers, no import: the schedules use them too."""

# step modes (SVDJ_STEP_*)
STEP_CROSS, STEP_FULL, STEP_CROSS_BIP, STEP_CROSS_ONLY, STEP_QUAD, STEP_QUAD_SECOND = range(6)
# matrix-core modes of the block apply (SVDJ_MMA_*), by config name
MMA_CODES = {"native": 0, "bf16x6": 1, "bf16x3": 2}
# mask and flags of svdj_block_steps' mma word (SVDJ_MMA_MASK, SVDJ_STEPS_*)
MMA_MASK, STEPS_GRAM2, STEPS_SHARED_GPU = 0xff, 0x100, 0x200
# inner orders by SVDJ_INNER_* code ("auto" follows them)
INNER_ORDERS = ("cyclic", "bipartite", "cross")
