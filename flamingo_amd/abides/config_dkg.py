"""DKG experiment driver (config/dkg.py surface).

    python -m flamingo_amd.abides -c dkg -n 60 [-s SEED] [--host_dkg] [-v]

The reference's construction (config/dkg.py): the service agent is agent 0, the n members are agents
1..n, and the cubic latency model connects them.  At the end the run prints whether every member
reported the same QUAL and the same group key, and checks that the key shares of degree + 1 members
interpolate to a key whose public point is that group key.  simulate() is the part a caller uses to
run a key generation inside a larger set-up (config_flamingo's --dkg).
"""
from __future__ import annotations

import argparse
from time import time

import numpy as np
import pandas as pd

from . import log
from .dkg import SA_ClientAgent as ClientAgent
from .dkg import SA_ServiceAgent as ServiceAgent
from .dkg import keygen
from .flamingo import protocol as param
from .kernel import Kernel
from .latency import LatencyModel
from .. import crypto as C


def parse(argv):
    ap = argparse.ArgumentParser(description="Detailed options for the DKG config.")
    ap.add_argument("-c", "--config", required=True)
    ap.add_argument("-k", "--skip_log", action="store_true")
    ap.add_argument("-l", "--log_dir", default=None)
    ap.add_argument("-n", "--num_clients", type=int, default=10)
    ap.add_argument("-s", "--seed", type=int, default=None)
    ap.add_argument("-v", "--verbose", action="store_true")
    ap.add_argument("--config_help", action="store_true")
    ap.add_argument("--latency", choices=("cubic", "deterministic"), default="cubic")
    # dealing and share checks per member on the host (keygen.configure(gpu_dkg=False)): same messages
    ap.add_argument("--host_dkg", action="store_true")
    args, _ = ap.parse_known_args(argv)
    return ap, args


def simulate(n: int, seed: int, latency: str = "cubic", poly_degree=None, client_cls=ClientAgent,
             skip_log: bool = True, log_dir=None, client_classes=None) -> dict:
    """One key generation among members 1..n -> {"members": {id: {"qual", "sk_share", "group_key"}},
    "server": the service agent, "agents": all agents, "state": the kernel's custom state}.
    client_classes: {id: class} for the members that are not client_cls (the tests' cheating dealers)."""
    rs = np.random.RandomState(seed)
    draw = lambda: np.random.RandomState(seed=rs.randint(low=0, high=2**32, dtype="uint64"))  # noqa: E731
    kernel = Kernel("DKG Kernel", random_state=draw())
    latency_rstate = draw()
    server = ServiceAgent(id=0, name="DKG Service Agent", type="ServiceAgent", random_state=draw(), msg_fwd_delay=0,
                          users=[*range(1, n + 1)], num_clients=n)
    agents = [server]
    for i in range(1, n + 1):
        cls = (client_classes or {}).get(i, client_cls)
        agents.append(cls(id=i, name=f"DKG Client Agent {i}", type="ClientAgent", num_clients=n,
                          random_state=draw(), poly_degree=poly_degree))
    pairwise = (len(agents), len(agents))
    model_args = {"connected": True, "min_latency": rs.uniform(low=10000000, high=100000000, size=pairwise),
                  "jitter": 0.3, "jitter_clip": 0.05, "jitter_unit": 5}
    model = LatencyModel(latency_model=latency, random_state=latency_rstate, kwargs=model_args)
    start = pd.to_datetime("2023-01-01")
    state = kernel.runner(agents=agents, startTime=start, stopTime=start + pd.to_timedelta("1:00:00"),
                          agentLatencyModel=model, defaultComputationDelay=int(1000000000 * 0.1),
                          skip_log=skip_log, log_dir=log_dir)
    return {"members": state.get("dkg", {}), "server": server, "agents": agents, "state": state}


def agreed(members: dict) -> tuple:
    """(QUAL, group key) when every member reported the same, else raises."""
    quals = {tuple(m["qual"]) for m in members.values()}
    keys = {m["group_key"] for m in members.values()}
    if len(quals) != 1 or len(keys) != 1:
        raise RuntimeError(f"the members disagree: {len(quals)} QUAL sets, {len(keys)} group keys")
    return list(quals.pop()), keys.pop()


def interpolated_key(members: dict, ids) -> int:
    """The secret key the shares of the members `ids` interpolate to (only a test or this driver's
    closing check ever puts that many shares in one place)."""
    from .flamingo.seeds import shamir_recover
    return shamir_recover([members[i]["sk_share"] for i in ids])


def run(argv=None):
    ap, args = parse(argv)
    if args.config_help:
        ap.print_help()
        return None
    seed = args.seed or int(pd.Timestamp.now().timestamp() * 1000000) % (2**32 - 1)
    log.silent_mode = not args.verbose
    n = args.num_clients
    if n < 2:
        raise ValueError("a key generation needs at least 2 members")
    keygen.configure(gpu_dkg=not args.host_dkg)
    path = "GPU" if keygen.on_gpu() else "host"
    print(f"Silent mode: {log.silent_mode}")
    print(f"Configuration seed: {seed}\n")
    t0 = time()
    res = simulate(n, seed, latency=args.latency, skip_log=args.skip_log, log_dir=args.log_dir)
    members = res["members"]
    qual, key = agreed(members)
    t = keygen.degree(n) + 1
    sk = interpolated_key(members, sorted(members)[:t])
    check = sum((a.elapsed_time["CHECK"] for a in res["agents"][1:]), pd.Timedelta(0)).total_seconds()
    print()
    print("######## Distributed key generation ########")
    print(f"    members: {n}, polynomial degree: {t - 1}, path: {path}")
    print(f"    members that finished: {len(members)}; all agree on QUAL ({len(qual)} dealers) and on one group key: True")
    print(f"    {t} key shares interpolate to the group key's secret: {C.mul(sk) == key}")
    print(f"    checking shares took {check:.3f} s over all members; wall {time() - t0:.1f} s")
    print()
    res["qual"], res["group_key"] = qual, key
    keygen.configure(gpu_dkg=True)
    return res
