"""The launches of a tick, observed: fb_timing_read's stage names and launch counts of every
case in tests/plan_cases.py equal the table (the same table tests/test_plan.py holds
plan_tick to on the CPU)."""
import pytest

import plan_cases as pc

pytestmark = pytest.mark.gpu


def _contexts(case):
    import torch  # noqa: F401  (loads the HIP runtime before libfaasbal)
    from faasbal import GpuBalancer
    from faasbal.sharded import ShardedBalancer

    st = pc.case_state(case["W"], case["free"], case["H"])
    cap = case["H"] + 4 * pc.MAX_EVENTS
    if case["kind"] == "shard":
        bals = [ShardedBalancer(r, 2, case["W"], cap, max_events=pc.MAX_EVENTS) for r in range(2)]
    else:
        bals = [GpuBalancer(case["W"], cap, max_events=pc.MAX_EVENTS,
                            mode="deque" if case["kind"] == "deque" else "heartbeat")]
    for b in bals:
        b.load(st)
        for k, v in case["knobs"].items():
            b.set_path(k, v)
        if case["window"]:
            b.set_window(case["window"])
    return bals


def _run(bals, W, op, T):
    """Launch ``op`` on every context (the sharded exchange summed on the device) and wait."""
    import torch

    if op == "read":
        for b in bals:
            b.read_state(with_log=False)
        return False
    for b in bals:
        if op == "purge":
            b._E = 0
            b._chk(b.lib.fb_purge_launch(b.h, pc.NOW, pc.TTE))
        elif op == "idle":
            b.launch(pc.NOW, pc.TTE, n_pending=T)
        else:
            b.launch(pc.NOW, pc.TTE, *pc.messages(W, op), n_pending=T)
    if len(bals) > 1:
        torch.cuda.synchronize()
        total = bals[0].exchange().clone()
        for b in bals[1:]:
            total += b.exchange()
        for b in bals:
            b.exchange().copy_(total)
        torch.cuda.synchronize()
        for b in bals:
            b.cont()
    for b in bals:
        b.wait()
    return True


def observe(case):
    """{stage: launches} of the case's measured operations (rank 0 of a sharded group)."""
    bals = _contexts(case)
    try:
        for op in case["history"]:
            if _run(bals, case["W"], op, 0):
                for b in bals:
                    b.commit()
        bals[0].timing_enable(True)
        bals[0].timing_read()
        for op in case["measure"]:
            _run(bals, case["W"], op, pc.T_MEASURE)
        return {k: int(v[1]) for k, v in bals[0].timing_read().items()}
    finally:
        for b in bals:
            b.close()


@pytest.mark.parametrize("name", [c["name"] for c in pc.CASES])
def test_launches_match_table(name):
    case = pc.BY_NAME[name]
    got = observe(case)
    print(name, got)
    assert got == case["expect"]
