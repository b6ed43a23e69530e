"""The trace launch's plan, restated from the contract csrc/pm_plan.h states
(TraceShape -> TracePlan) and from the LDS layout the kernels index
(pm_trace.hip): integers only. tests/test_trace_plan.py holds
csrc/pm_plan.cpp's plan_trace equal to it."""

TRACE_BLOCK, HOLD_MPC, HOLD_WORDS = 256, 4, 27
WAVES_PER_BLOCK = TRACE_BLOCK // 64
MODE_GLOBAL, MODE_LDS, MODE_BRUTE, MODE_INST = 0, 1, 2, 3
LANE_GLOBAL, LANE_LDS, LANE_BRUTE, LANE_INST, POOL, POOL8 = range(6)
LANE_OF_MODE = {MODE_GLOBAL: LANE_GLOBAL, MODE_LDS: LANE_LDS, MODE_BRUTE: LANE_BRUTE, MODE_INST: LANE_INST}
HELD_BYTES = HOLD_WORDS * TRACE_BLOCK * 4  # a column of HOLD_WORDS words per thread


def ceil_div(a, b):
    return -(-a // b)


def stacks(entries):
    """a column of 4-byte stack entries per thread"""
    return entries * TRACE_BLOCK * 4


def lane_block_lds(depth, blob, held):
    """per-lane kernels: [stacks][scene blob][pad to 16 B][held columns]"""
    return stacks(depth) + (ceil_div(blob, 16) * 16 + HELD_BYTES if held else blob)


def table(cap, regs):
    """the occupancy model of tests/native/trace_plan_check.cpp: cap bytes of
    LDS per CU (0: unknown), regs[2 f + hold] register-bound waves per CU"""
    def ask(family, hold, lds):
        if cap == 0:
            return 0
        blocks = regs[2 * family + hold] // WAVES_PER_BLOCK
        return min(blocks, cap // lds if lds else blocks) * WAVES_PER_BLOCK
    return ask


def plan(paths, mpc, aligned, mode, wide, depth, blob, pool_stack, trace_pool, trace_hold, cus, ask):
    """-> (plan dict, [(family, hold, lds) asked, in order])"""
    asked = []

    def waves(family, hold, lds):
        asked.append((family, hold, lds))
        return ask(family, hold, lds)

    want_hold = bool(trace_hold)
    p = dict(lstk=0, pool_paths=0, spill_entries=0, spill_stride=0)
    pooled = False
    if not wide:
        if want_hold:
            # a per-lane MODE_INST launch asks for the MODE_GLOBAL kernel's occupancy
            fam = LANE_GLOBAL if mode == MODE_INST else LANE_OF_MODE[mode]
            held = waves(fam, 1, lane_block_lds(depth, blob, True))
            plain = waves(fam, 0, lane_block_lds(depth, blob, False))
            want_hold = held >= plain
    else:
        fam = POOL8 if wide == 3 else POOL
        lstk = pool_stack if 0 < pool_stack < depth else depth
        # the pooled occupancy is asked with the scene's LDS bytes on top of the stacks
        per_cu = waves(fam, 0, stacks(lstk) + blob)
        if want_hold:
            held = waves(fam, 1, stacks(lstk) + blob + HELD_BYTES)
            want_hold = held >= per_cu
            if want_hold:
                per_cu = held
        round_waves = (cus if cus > 0 else 256) * (per_cu if per_cu > 0 else 16)
        per_wave = max(1, ceil_div(paths, round_waves))
        pool_blocks = ceil_div(ceil_div(paths, per_wave), WAVES_PER_BLOCK)
        p["lstk"] = lstk
        p["pool_paths"] = per_wave if (trace_pool or wide == 3) else 0
        if lstk < depth:
            p["spill_entries"] = depth - lstk
            p["spill_stride"] = pool_blocks * TRACE_BLOCK
        pooled = p["pool_paths"] > 0 and mode == MODE_GLOBAL
        if pooled:
            p.update(family=fam, grid=pool_blocks, lds=stacks(lstk), lds_hold=stacks(lstk) + HELD_BYTES)
    if not pooled:
        p.update(family=LANE_OF_MODE[mode], grid=ceil_div(paths, TRACE_BLOCK), lds=lane_block_lds(depth, blob, False),
                 lds_hold=lane_block_lds(depth, blob, True))
    p["pooled"] = int(pooled)
    p["hold"] = int(want_hold)
    p["hold_launch"] = int(want_hold and mpc == HOLD_MPC and bool(aligned))
    return p, asked


def pool_layout(p, paths):
    """how a pooled plan's waves share `paths` (trace_pool_body: wave w takes [w * pool_paths, (w + 1) * pool_paths)
    clipped by paths): (waves with a pool, paths of the last pool, waves of the last block whose pool is empty)"""
    assert p["pooled"] and p["pool_paths"] > 0
    waves = ceil_div(paths, p["pool_paths"])
    return waves, paths - (waves - 1) * p["pool_paths"], p["grid"] * WAVES_PER_BLOCK - waves
