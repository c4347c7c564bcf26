"""Cost model of march_kernel's scheduling: how many wave-level VALU instructions a ray costs under a scheduling
policy, given the measured per-phase instruction counts and the measured transition rates of a configuration.
Planning tool only (no GPU, no oracle): rays are a Markov chain MARCH -> {MARCH, HIT, ENDED}, HIT -> {MARCH, ENDED}
with the rates of tools/diag_march.py; a workgroup's waves advance in parallel, each paying the wave-level cost of the
body it executes whatever the number of active lanes.

    python tools/sim_pool.py [c3|c5]
    python tools/sim_pool.py passes [c3|c5]     march_pool_kernel's shipped pass policy and its fused passes (VRT_POOL_FUSE)
    python tools/sim_pool.py passes [c3|c5] --early-end    ... with a ray ENDED by the step that uses up its life
"""
import random
import sys

CFG = {
    # p_hit / p_end: per march iteration; p_break: per hit           (profiles/r03_diag_c3.txt, r03_diag_c5.txt)
    "c3": dict(p_hit=0.356, p_end=0.166, p_break=0.20),
    "c5": dict(p_hit=0.167, p_end=0.0053, p_break=0.07),
}
# wave-level VALU instructions per execution of a body (static counts of the shipped kernel's ISA, hot path)
COST = dict(march=310, hit=350, end=100, refill=150, pass_=40, xchg=30)

M, H, E, I = 0, 1, 2, 3


class Ray:
    __slots__ = ("state",)

    def __init__(self):
        self.state = M


def step_march(ray, c, rng):
    u = rng.random()
    if u < c["p_hit"]:
        ray.state = H
    elif u < c["p_hit"] + c["p_end"]:
        ray.state = E


def step_hit(ray, c, rng):
    ray.state = E if rng.random() < c["p_break"] else M


def baseline(c, rng, n_rays=200000, t_hit=24, t_end=32, max_iters=3):
    """the shipped policy: one ray per lane, thresholds"""
    lanes = [None] * 64
    done = 0
    cost = 0
    lane_sum = {"march": 0, "hit": 0, "end": 0, "refill": 0}
    execs = {"march": 0, "hit": 0, "end": 0, "refill": 0}
    issued = 0
    while done < n_rays:
        cost += COST["pass_"]
        idle = [i for i in range(64) if lanes[i] is None]
        if idle and issued < n_rays:
            cost += COST["refill"]
            execs["refill"] += 1
            lane_sum["refill"] += len(idle)
            for i in idle:
                lanes[i] = Ray()
                issued += 1
        iters = 0
        while True:
            nm = sum(1 for r in lanes if r and r.state == M)
            nh = sum(1 for r in lanes if r and r.state == H)
            ne = sum(1 for r in lanes if r and r.state == E)
            if nm == 0 or nh >= t_hit or ne >= t_end:
                break
            if iters >= max_iters and nh + ne > 0:
                break
            iters += 1
            cost += COST["march"]
            execs["march"] += 1
            lane_sum["march"] += nm
            for r in lanes:
                if r and r.state == M:
                    step_march(r, c, rng)
        nm = sum(1 for r in lanes if r and r.state == M)
        nh = sum(1 for r in lanes if r and r.state == H)
        capped = iters >= max_iters
        if nh and (nm == 0 or capped or nh >= t_hit):
            cost += COST["hit"]
            execs["hit"] += 1
            lane_sum["hit"] += nh
            for r in lanes:
                if r and r.state == H:
                    step_hit(r, c, rng)
        nm = sum(1 for r in lanes if r and r.state == M)
        ne = sum(1 for r in lanes if r and r.state == E)
        if ne and (nm == 0 or capped or ne >= t_end):
            cost += COST["end"]
            execs["end"] += 1
            lane_sum["end"] += ne
            for i in range(64):
                if lanes[i] and lanes[i].state == E:
                    lanes[i] = None
                    done += 1
    return cost / done, {k: lane_sum[k] / max(1, execs[k]) for k in execs}


def private_pool(c, rng, parked=48, n_rays=200000, t_hit=56, t_end=56, swap_min=8):
    """wave-private pool: 64 lanes + `parked` slots in LDS, no cross-wave traffic.  Before a body runs, lanes whose ray
    is in another state swap with parked rays in the wanted state."""
    lanes = [None] * 64
    park = []
    done = issued = 0
    cost = 0
    lane_sum = {"march": 0, "hit": 0, "end": 0, "refill": 0}
    execs = {"march": 0, "hit": 0, "end": 0, "refill": 0, "xchg": 0}
    moved = 0

    def count(st):
        return sum(1 for r in lanes if r and r.state == st), sum(1 for r in park if r.state == st)

    def gather(st):
        """bring parked rays of state st into lanes that hold something else (or nothing)"""
        nonlocal cost, moved
        src = [r for r in park if r.state == st]
        if not src:
            return
        # empty lanes first, then lanes in other states while there is room to park them
        targets = [i for i in range(64) if lanes[i] is None] + [i for i in range(64) if lanes[i] and lanes[i].state != st]
        n = 0
        for i in targets:
            if not src:
                break
            r = src.pop()
            park.remove(r)
            if lanes[i] is not None:
                park.append(lanes[i])
            lanes[i] = r
            n += 1
        if n:
            cost += COST["xchg"]
            execs["xchg"] += 1
            moved += n

    while done < n_rays:
        cost += COST["pass_"]
        lm, pm = count(M)
        lh, ph = count(H)
        le, pe = count(E)
        nidle = sum(1 for r in lanes if r is None)
        total = 64 - nidle + len(park)
        # choose the body with the most rays available, preferring the expensive waits
        if lh + ph >= min(t_hit, total) and lh + ph > 0:
            if ph >= swap_min or lh < 64:
                gather(H)
            n = sum(1 for r in lanes if r and r.state == H)
            cost += COST["hit"]
            execs["hit"] += 1
            lane_sum["hit"] += n
            for r in lanes:
                if r and r.state == H:
                    step_hit(r, c, rng)
            continue
        if le + pe >= min(t_end, total) and le + pe > 0:
            gather(E)
            n = sum(1 for r in lanes if r and r.state == E)
            cost += COST["end"]
            execs["end"] += 1
            lane_sum["end"] += n
            for i in range(64):
                if lanes[i] and lanes[i].state == E:
                    lanes[i] = None
                    done += 1
            idle = [i for i in range(64) if lanes[i] is None]
            if idle and issued < n_rays + 64:
                cost += COST["refill"]
                execs["refill"] += 1
                lane_sum["refill"] += len(idle)
                for i in idle:
                    lanes[i] = Ray()
                    issued += 1
            continue
        # march: park waiting lanes if there is room and marching rays to bring in
        if pm > 0 or nidle > 0:
            # make room: park H/E lanes (each park of a lane ray needs a free slot)
            free = parked - len(park)
            waiting = [i for i in range(64) if lanes[i] and lanes[i].state != M]
            n = 0
            src = [r for r in park if r.state == M]
            for i in waiting:
                if not src:
                    break
                r = src.pop()
                park.remove(r)
                park.append(lanes[i])
                lanes[i] = r
                n += 1
            for i in range(64):
                if lanes[i] is None and src:
                    r = src.pop()
                    park.remove(r)
                    lanes[i] = r
                    n += 1
            if n:
                cost += COST["xchg"]
                execs["xchg"] += 1
                moved += n
        # still idle lanes or lanes waiting with free parking: take fresh rays into them
        free = parked - len(park)
        waiting = [i for i in range(64) if lanes[i] and lanes[i].state != M]
        evict = waiting[:free]
        if evict:
            for i in evict:
                park.append(lanes[i])
                lanes[i] = None
            cost += COST["xchg"]
            execs["xchg"] += 1
            moved += len(evict)
        idle = [i for i in range(64) if lanes[i] is None]
        if idle and issued < n_rays + 64:
            cost += COST["refill"]
            execs["refill"] += 1
            lane_sum["refill"] += len(idle)
            for i in idle:
                lanes[i] = Ray()
                issued += 1
        nm = sum(1 for r in lanes if r and r.state == M)
        if nm == 0:
            # nothing marches: run whatever waits
            lh, ph = count(H)
            if lh + ph:
                gather(H)
                n = sum(1 for r in lanes if r and r.state == H)
                cost += COST["hit"]
                execs["hit"] += 1
                lane_sum["hit"] += n
                for r in lanes:
                    if r and r.state == H:
                        step_hit(r, c, rng)
            else:
                gather(E)
                n = sum(1 for r in lanes if r and r.state == E)
                if n == 0:
                    break
                cost += COST["end"]
                execs["end"] += 1
                lane_sum["end"] += n
                for i in range(64):
                    if lanes[i] and lanes[i].state == E:
                        lanes[i] = None
                        done += 1
            continue
        cost += COST["march"]
        execs["march"] += 1
        lane_sum["march"] += nm
        for r in lanes:
            if r and r.state == M:
                step_march(r, c, rng)
    out = {k: lane_sum[k] / max(1, execs[k]) for k in lane_sum}
    out["xchg/ray"] = execs["xchg"] / done
    out["moved/ray"] = moved / done
    return cost / done, out


def early_end_rates(c):
    """The chain's rates when the loop condition is decided at the end of the step that uses up the ray's life (march_step,
    hit_body: LANE_ENDED straight after the advance) instead of by an iteration of its own.  The measured rates are per march
    iteration, "end" iterations included: from MARCH a ray comes back to MARCH with rho0 = p_hit (1 - p_break) + 1 - p_hit -
    p_end, so it spends N = 1 / (1 - rho0) iterations, N (1 - p_end) of them on a step that does something.  Of those steps
    a = p_hit / (1 - p_end) find a voxel.  A ray that goes on after a step or a hit is dead with probability x, and x is what
    leaves the number of working steps per ray where it was: (1 - x)(1 - a p_break) = 1 - 1 / (N (1 - p_end)).  A fresh ray is
    alive.  Returns (a, x); config 3: 0.427, 0.218."""
    rho0 = c["p_hit"] * (1 - c["p_break"]) + 1 - c["p_hit"] - c["p_end"]
    work = (1 - c["p_end"]) / (1 - rho0)
    a = c["p_hit"] / (1 - c["p_end"])
    return a, 1 - (1 - 1 / work) / (1 - a * c["p_break"])


def shipped_pool(c, rng, fuse=0, slots=48, n_rays=200000, t_hit=40, t_end=60, swap_min=8, refill_min=8, keep=40, max_iters=3,
                 early_end=False):
    """march_pool_kernel's pass loop as shipped (python_raytracer_amd/csrc/vrt_kernels.hip): one target per pass -- HIT once
    t_hit rays wait anywhere in the wave's 64 lanes + `slots` parked places, ENDED (+ refill) once t_end do, else MARCH --,
    the exchange that brings rays of the target's state into the lanes (or parks waiting rays in free slots for fresh ones),
    then the bodies in source order.  fuse: -DVRT_POOL_FUSE's bits -- 1: an ENDED pass enters the march loop after its refill
    once `keep` lanes march; 2: the HIT body runs before the march loop and a HIT pass enters it under the same rule.
    Without rays left to hand out every pass runs all three bodies (tail mode).  early_end: a ray whose life a march step or
    the HIT body's advance used up is ENDED at the end of that step (early_end_rates) instead of marching once more to find
    out.  Counts, not costs: passes, executions of each body and the lanes they find."""
    a_hit, x_dead = early_end_rates(c) if early_end else (0.0, 0.0)
    lanes = [None] * 64      # a lane's state, or None
    park = []                # states of the parked rays
    done = issued = passes = 0
    execs = {"march": 0, "hit": 0, "end": 0, "refill": 0, "xchg": 0}
    lane_sum = {"march": 0, "hit": 0, "end": 0, "refill": 0, "xchg": 0}

    def hit_body(st):
        if rng.random() < c["p_break"]:
            return E
        return E if early_end and rng.random() < x_dead else M

    def march_body(st):
        u = rng.random()
        if early_end:
            return H if u < a_hit else (E if rng.random() < x_dead else M)
        return H if u < c["p_hit"] else (E if u < c["p_hit"] + c["p_end"] else M)

    def run(name, state, body):
        n = 0
        for i in range(64):
            if lanes[i] == state:
                lanes[i] = body(state)
                n += 1
        if n:
            execs[name] += 1
            lane_sum[name] += n
        return n

    while True:
        passes += 1
        n = {st: lanes.count(st) + park.count(st) for st in (M, H, E)}
        idle = lanes.count(None)
        rays_left = issued < n_rays
        can_add = rays_left and (idle > 0 or len(park) < slots)
        if rays_left:
            if n[H] >= t_hit:
                target = H
            elif n[E] >= t_end:
                target = E
            elif n[M] > 0 or can_add:
                target = M
            else:
                target = H if n[H] >= n[E] else E
        else:
            if n[M] + n[H] + n[E] == 0:
                break
            target = M
        tail = not rays_left
        # the exchange: lanes that hold another state first, then idle lanes, take the parked rays of the target's state; under
        # MARCH the ray holders left over park their rays in free slots and go idle (for a fresh ray)
        wanted = (lambda st: st is not None) if tail else (lambda st: st == target)
        others = [i for i in range(64) if lanes[i] is not None and not wanted(lanes[i])] + [i for i in range(64) if lanes[i] is None]
        n_a = 64 - idle - sum(1 for st in lanes if st is not None and wanted(st))
        src = [k for k, st in enumerate(park) if wanted(st)]
        take = min(len(others), len(src))
        free = slots - len(park)
        evict = min(max(n_a - len(src), 0), free) if (target == M and rays_left and not tail) else 0
        in_lanes = sum(1 for st in lanes if st is not None and wanted(st))
        if take + evict >= (1 if tail else swap_min) or (take + evict > 0 and in_lanes == 0):
            execs["xchg"] += 1
            lane_sum["xchg"] += take + evict
            for i, k in zip(others[:take], src[:take]):
                lanes[i], park[k] = park[k], lanes[i]
            park[:] = [st for st in park if st is not None]
            for i in others[take:take + evict]:
                park.append(lanes[i])
                lanes[i] = None
        if tail or target == E:
            k = run("end", E, lambda st: None)
            done += k
        if target != H and issued < n_rays:
            idle_now = [i for i in range(64) if lanes[i] is None]
            if idle_now and (target == E or len(idle_now) >= refill_min or lanes.count(M) == 0):
                take_n = min(len(idle_now), n_rays - issued)
                for i in idle_now[:take_n]:
                    lanes[i] = M
                issued += take_n
                execs["refill"] += 1
                lane_sum["refill"] += take_n
        if (fuse & 2) and (tail or target == H):
            run("hit", H, hit_body)
        fed = ((fuse & 1) and target == E) or ((fuse & 2) and target == H)
        if target == M or fed:
            for it in range(1 if tail else max_iters):
                m = lanes.count(M)
                if m == 0 or ((it > 0 or fed) and m < keep):
                    break
                run("march", M, march_body)
        if not (fuse & 2) and (tail or target == H):
            run("hit", H, hit_body)
    out = {k: round(lane_sum[k] / max(1, execs[k]), 1) for k in lane_sum}
    return passes * 64 / done, {k: execs[k] * 64 / done for k in execs}, out


def passes_table(name, early_end=False):
    c = CFG[name]
    pol = dict(c3=(40, 60, 8, 8, 40, 3), c5=(48, 32, 4, 8, 40, 5))[name]   # pool_policy's defaults
    base = None
    print("%s, shipped knobs %s, 48 slots; per ray x 64%s" % (name, " / ".join(str(v) for v in pol),
          "; the loop condition decided at the end of the step (hit %.3f per working step, dead %.3f of the rays that go on)"
          % early_end_rates(c) if early_end else ""))
    for fuse, label in ((0, "shipped"), (1, "ENDED + refill falls into the march"), (2, "HIT falls into the march"), (3, "both")):
        p, ex, ln = shipped_pool(c, random.Random(1), fuse=fuse, t_hit=pol[0], t_end=pol[1], swap_min=pol[2], refill_min=pol[3],
                                 keep=pol[4], max_iters=pol[5], early_end=early_end)
        base = base or (p, ex["march"])
        print("fuse %d  %-36s passes %5.2f (%+5.1f%%)  march steps %5.2f (%+5.1f%%) at %4.1f lanes  hit %4.2f at %4.1f  ended %4.2f at %4.1f  exchanges %4.2f" % (
            fuse, label, p, 100 * (p / base[0] - 1), ex["march"], 100 * (ex["march"] / base[1] - 1), ln["march"], ex["hit"], ln["hit"],
            ex["end"], ln["end"], ex["xchg"]))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "passes":
        args = [a for a in sys.argv[2:] if a != "--early-end"]
        passes_table(args[0] if args else "c3", early_end="--early-end" in sys.argv[2:])
        sys.exit(0)
    name = sys.argv[1] if len(sys.argv) > 1 else "c3"
    c = CFG[name]
    rng = random.Random(1)
    pol = dict(c3=(24, 32, 3), c5=(24, 24, 5))[name]
    b, lanes = baseline(c, rng, t_hit=pol[0], t_end=pol[1], max_iters=pol[2])
    print("%s baseline: %.1f wave-VALU per ray; lanes %s" % (name, b, {k: round(v, 1) for k, v in lanes.items()}))
    for parked in (16, 32, 48, 64, 96):
        for th in (40, 48, 56, 64):
            v, lanes = private_pool(c, rng, parked=parked, t_hit=th, t_end=th)
            print("private pool %3d parked, threshold %2d: %.1f (%.2fx)  %s" % (
                parked, th, v, b / v, {k: round(x, 2) for k, x in lanes.items()}))
