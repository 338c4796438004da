#!/usr/bin/env python3
"""Rates of the rollout entry points at the headline shape (65 536 envs x 24x24, mode None, attached int8 codes), one process,
the variants alternated so that they share the clocks:

  tape      VecTron.rollout_actions, 64-step launches walking a random tape that lives in HBM (2 bytes per env-step)
  per_step  the same rows through tron_step_encode, one launch per step: what a caller with its own actions had before
  tape_rec  the tape launches with all three records (reward, done, winner: 10 bytes stored per env-step) into a resident
            record buffer of --tape-steps rows
  tape_dw   tape_rec without the reward tape (done and winner only: 2 bytes stored per env-step)
  per_step_rec  the same record rows through tron_step_encode with its three outputs pointed at them, one launch per step:
            what a caller who wanted the records had before
  rand64    tron_rollout_random, 64 steps per launch
  rand20    tron_rollout_random, 20 steps per launch

A train is --steps env-steps per env, timed by the host clock between two device synchronisations; every variant is warmed
up, then --repeats rounds run the variants one after the other.  Prints one line per variant (median, min, max over the
rounds, G env-steps/s) and one JSON line.  TRON_HIP_LIB selects the library: with one that has no tron_rollout_actions (a
build of an older commit, for the comparison of rand64 / rand20) the tape variant is left out and said so; with one that has
no tron_rollout_actions_records, tape_rec, tape_dw and per_step_rec are.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-q-learning_tron_amd"))

import torch  # noqa: E402
import tron.vec as tv  # noqa: E402

nat = tv.nat                                                     # the ctypes binding (tron/_native.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--width", type=int, default=24)
    ap.add_argument("--steps", type=int, default=12800, help="env-steps per env and train (a multiple of 64 and 20)")
    ap.add_argument("--tape-steps", type=int, default=2048, help="rows of the resident tape (a multiple of 64)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=4, help="warm-up trains of 320 steps per variant")
    a = ap.parse_args()
    assert a.steps % 64 == 0 and a.steps % 20 == 0 and a.tape_steps % 64 == 0
    if not torch.cuda.is_available():
        sys.exit("roll_actions_bench.py measures on the GPU; none here")

    have_tape = hasattr(C.CDLL(nat.LIB_PATH), "tron_rollout_actions")
    have_rec = hasattr(C.CDLL(nat.LIB_PATH), "tron_rollout_actions_records")
    if not have_tape:
        nat.SIGNATURES.pop("tron_rollout_actions")               # an older library: bind what it has
    if not have_rec:
        nat.SIGNATURES.pop("tron_rollout_actions_records")
    N = a.envs
    env = tv.VecTron(N, a.width, seed=0x5EED, rank=0, obs_format="codes")
    assert env.obs_is_state
    env.reset()
    tape = torch.randint(0, 4, (a.tape_steps, N, 2), dtype=torch.int8, device="cuda")
    lib, h, stream = env._lib, env._h, nat.stream_ptr()
    row_bytes = 2 * N
    base = tape.data_ptr()
    step_args = [(h, C.c_void_p(base + k * row_bytes), None, nat.STEP_AUTORESET, env._fmt, nat.ptr(env.obs), nat.ptr(env.done),
                  nat.ptr(env.winner), nat.ptr(env.reward), stream) for k in range(a.tape_steps)]

    if have_rec:                                                 # the resident record tapes, row k beside the tape's row k
        rec = (torch.empty(a.tape_steps, N, 2, dtype=torch.float32, device="cuda"),
               torch.empty(a.tape_steps, N, dtype=torch.int8, device="cuda"),
               torch.empty(a.tape_steps, N, dtype=torch.int8, device="cuda"))
        step_rec_args = [(h, C.c_void_p(base + k * row_bytes), None, nat.STEP_AUTORESET, env._fmt, nat.ptr(env.obs),
                          C.c_void_p(rec[1].data_ptr() + k * N), C.c_void_p(rec[2].data_ptr() + k * N),
                          C.c_void_p(rec[0].data_ptr() + k * 8 * N), stream) for k in range(a.tape_steps)]

    def run_tape_rec(steps):
        for j in range(steps // 64):
            r = (j * 64) % a.tape_steps
            env.rollout_actions(tape[r:r + 64], records=(rec[0][r:r + 64], rec[1][r:r + 64], rec[2][r:r + 64]))

    def run_tape_dw(steps):
        for j in range(steps // 64):
            r = (j * 64) % a.tape_steps
            env.rollout_actions(tape[r:r + 64], records=(None, rec[1][r:r + 64], rec[2][r:r + 64]))

    def run_per_step_rec(steps):
        fn = lib.tron_step_encode
        for k in range(steps):
            rc = fn(*step_rec_args[k % a.tape_steps])
            if rc:
                nat.check(rc, "tron_step_encode")

    def run_tape(steps):
        for j in range(steps // 64):
            r = (j * 64) % a.tape_steps
            env.rollout_actions(tape[r:r + 64])

    def run_per_step(steps):
        fn = lib.tron_step_encode
        for k in range(steps):
            rc = fn(*step_args[k % a.tape_steps])
            if rc:
                nat.check(rc, "tron_step_encode")

    def run_random(per_launch):
        def run(steps):
            for _ in range(steps // per_launch):
                env.rollout_random(per_launch)
        return run

    variants = [("tape", run_tape)] if have_tape else []
    variants += [("per_step", run_per_step)]
    if have_rec:
        variants += [("tape_rec", run_tape_rec), ("tape_dw", run_tape_dw), ("per_step_rec", run_per_step_rec)]
    variants += [("rand64", run_random(64)), ("rand20", run_random(20))]
    for _, fn in variants:
        fn(320 * a.warmup)
    torch.cuda.synchronize()
    rates = {name: [] for name, _ in variants}
    for _ in range(a.repeats):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(a.steps)
            torch.cuda.synchronize()
            rates[name].append(N * a.steps / (time.perf_counter() - t0))
    print(f"{os.path.basename(os.path.dirname(nat.LIB_PATH)) or '.'}/{os.path.basename(nat.LIB_PATH)}: {N} envs x {a.width}x{a.width}, "
          f"trains of {a.steps} steps, {a.repeats} rounds, G env-steps/s: median [min max]")
    if not have_tape:
        print("  tape      not in this library")
    if not have_rec:
        print("  tape_rec, tape_dw, per_step_rec  not in this library (no tron_rollout_actions_records)")
    for name, _ in variants:
        r = [x / 1e9 for x in rates[name]]
        print(f"  {name:12s} {statistics.median(r):7.3f} [{min(r):7.3f} {max(r):7.3f}]", flush=True)
    print(json.dumps({"lib": nat.LIB_PATH, "envs": N, "width": a.width, "steps": a.steps, "rates": rates}))
    env.close()


if __name__ == "__main__":
    main()
