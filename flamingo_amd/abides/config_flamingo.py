"""Flamingo experiment driver (config/flamingo.py surface).

    python -m flamingo_amd.abides -c flamingo -n 128 -i 1 [-o 1] [-s SEED] [-v]

Same flags as the reference (config/flamingo.py:24-52), same agent
construction (:179-215), cubic latency model (:225-238) and result print
(:253-266).  Extra flags: --vector_len (reference constant 16000,
util/param.py:8), --root_seed_hex (the reference draws it at random,
util/param.py:31), --offline id,id,... (clients that crash before sending in
every iteration: explicit dropout injection), --dropout F (in each iteration t a
fresh offline set PCG64(seed=t).choice(N, round(F N), replace=False), SURVEY 8d's
c5 recipe: BASELINE c5 is -n 4096 --vector_len 1048576 -i 10 --dropout 0.01),
--latency deterministic (model/LatencyModel.py:142-143: min latency only, so no
VECTOR arrives late and the offline sets are exactly the injected ones; the
reference config's cubic model, the default, adds emergent late-message dropouts).
At the end the run prints, per iteration, |U| and whether final_sum == |U| in
every slot (the all-ones known answer, SA_ClientAgent.py:304 + SA_ServiceAgent.py:605).
"""
from __future__ import annotations

import argparse
import gc
from datetime import timedelta
from time import time

import numpy as np
import pandas as pd

from . import log
from .kernel import Kernel
from .latency import LatencyModel
from .flamingo import SA_ClientAgent as ClientAgent
from .flamingo import SA_ServiceAgent as ServiceAgent
from .flamingo import protocol as param
from .. import params as P


def parse(argv):
    ap = argparse.ArgumentParser(description="Detailed options for the Flamingo config.")
    ap.add_argument("-a", "--clear_learning", action="store_true")
    ap.add_argument("-c", "--config", required=True)
    ap.add_argument("-i", "--num_iterations", type=int, default=5)
    ap.add_argument("-k", "--skip_log", action="store_true")
    ap.add_argument("-l", "--log_dir", default=None)
    ap.add_argument("-n", "--num_clients", type=int, default=5)
    ap.add_argument("-o", "--neighborhood_size", type=int, default=1)
    ap.add_argument("--round_time", type=int, default=10)
    ap.add_argument("-s", "--seed", type=int, default=None)
    ap.add_argument("-v", "--verbose", action="store_true")
    ap.add_argument("-p", "--parallel_mode", type=bool, default=True)   # type=bool quirk kept
    ap.add_argument("-d", "--debug_mode", type=bool, default=False)
    ap.add_argument("--config_help", action="store_true")
    ap.add_argument("--vector_len", type=int, default=P.vector_len)
    ap.add_argument("--root_seed_hex", default=None)
    ap.add_argument("--offline", default="")
    ap.add_argument("--dropout", type=float, default=0.0)
    ap.add_argument("--latency", choices=("cubic", "deterministic"), default="cubic")
    ap.add_argument("--committee_size", type=int, default=P.committee_size)
    # the clients' m_i dealing and AES-GCM sealing per client on the host, not batched on the GPU
    # (protocol.configure(gpu_deal=False)): same messages, for A/B timing
    ap.add_argument("--host_deal", action="store_true")
    # committee members verify the signatures forwarded in DEC before they release decryption shares
    # (protocol.configure(check_signatures=True)); off by default
    ap.add_argument("--check_signatures", action="store_true")
    # ... in one GPU call per member (protocol.configure(gpu_verify=True)), not row by row on the host
    # (OpenSSL), which is the default: same verdicts, no faster at a member's 61 rows
    ap.add_argument("--gpu_verify", action="store_true")
    # the sealed m_i shares keep their AES-GCM tag and the committee verifies it before it opens them
    # (protocol.configure(authenticate_shares=True)); off by default
    ap.add_argument("--authenticate_shares", action="store_true")
    # the committee generates the system key itself before the first iteration, by the DKG of
    # abides/dkg among its sorted members (protocol.configure(dkg=True)): the server never holds the key
    # and sends no COMMITTEE_SHARED_SK; off by default.  --host_dkg: that DKG's dealing and checks on the host
    ap.add_argument("--dkg", action="store_true")
    ap.add_argument("--host_dkg", action="store_true")
    # the clients' inputs are float32 updates, encoded in fixed point inside the masking kernel, and the server
    # also decodes the sum to final_mean (protocol.configure(codec=...)): F fractional bits, clip CLIP, nearest-even
    # rounding or, with ",sr", stochastic rounding; ",pack2" or ",pack4": that many parameters per ring word (the
    # packed codec: n 2 ceil(CLIP 2^F) must fit 16 or 8 bits, so pack4 serves small cohorts only); off by default
    ap.add_argument("--float_inputs", default=None, metavar="F,CLIP[,sr][,pack2|pack4]")
    # distributed differential privacy: every client adds a share of binomial noise, BITS fair coins per parameter
    # (even, 2..1024), to its quantised update inside the masking kernel (protocol.configure(dp_noise=...)); needs
    # --float_inputs, and headroom for n (ceil(CLIP 2^F) + BITS / 2); turning BITS into an (epsilon, delta) is the
    # caller's business; off by default
    ap.add_argument("--dp_noise", type=int, default=0, metavar="BITS")
    # ... or a share of discrete Gaussian noise of parameter SIGMA truncated to +-TAIL (an integer in 1..512, default
    # ceil(10 SIGMA)), sampled from a cumulative table inside the same kernel (protocol.configure(dp_gauss=...)); needs
    # --float_inputs and headroom for n (ceil(CLIP 2^F) + TAIL); not together with --dp_noise; the accounting (SIGMA, the
    # sensitivity of --round_bound, dgauss.tail_mass for delta) is the caller's business; off by default
    ap.add_argument("--dp_gauss", default=None, metavar="SIGMA[,TAIL]")
    # every client rotates its float update by a randomised Hadamard transform in blocks of 2^LOG2BLOCK parameters
    # (4..12) before the encode, under a public key per iteration, and the server rotates the decoded mean back
    # (protocol.configure(rotate=...)): CLIP then bounds the rotated coordinates, about ||x||_2 / 2^(LOG2BLOCK / 2)
    # per block where it had to cover the largest coordinate; needs --float_inputs; off by default
    ap.add_argument("--rotate", type=int, default=0, metavar="LOG2BLOCK")
    # every client scales its float update to an L2 norm of at most C before the rotation, or in the rotation's own
    # pass with --rotate (protocol.configure(l2_clip=...)): one client then moves the sum by at most C in L2, the
    # sensitivity --dp_noise is measured against; turning C into a privacy statement is the caller's business; needs
    # --float_inputs; off by default
    ap.add_argument("--l2_clip", type=float, default=0.0, metavar="C")
    # conditional stochastic rounding: every client draws ATTEMPTS (1..8, default 4) candidate dither seeds a batch and
    # rounds with the first whose integer row has a sum of squares within Delta^2 = MaskEngine.round_bound(C, F, d,
    # TAIL), TAIL = k = sqrt(2 ln(1 / beta)) for a per-draw failure probability beta (protocol.configure(round_bound=
    # ...)): Delta / 2^F is then the L2 sensitivity of the sum to one client after rounding, where C is the one before
    # it; needs --float_inputs F,CLIP,sr and --l2_clip; 0 turns it off; off by default
    ap.add_argument("--round_bound", default=None, metavar="TAIL[,ATTEMPTS]")
    # the server decodes the packed sum modulo the field, following the carries from one field into the next
    # (protocol.configure(modular=...)): it admits n by MaskEngine.codec_check_modular where the worst-case headroom rule
    # refuses it, and reports how many centred sums reached ceil(FRACTION H), H = 2^(32/pack - 1), and the largest;
    # FRACTION in (0, 1]; the library bounds no wrap probability: that and any (epsilon, delta) are the caller's business;
    # needs --float_inputs with pack2 or pack4; the clients are unchanged; off by default
    ap.add_argument("--modular", type=float, default=0.0, metavar="FRACTION")
    args, _ = ap.parse_known_args(argv)
    return ap, args


def parse_float_inputs(spec):
    """"F,CLIP" or "F,CLIP,sr" -> (frac_bits, clip, "nearest" | "stochastic"); with a last ",pack2" or ",pack4"
    -> (frac_bits, clip, rounding, 2 | 4); None or "" -> False (off)."""
    if not spec:
        return False
    parts = [s.strip() for s in spec.split(",")]
    pack = None
    if len(parts) > 2 and parts[-1] in ("pack2", "pack4"):
        pack = int(parts.pop()[4:])
    if len(parts) not in (2, 3) or (len(parts) == 3 and parts[2] != "sr"):
        raise ValueError("--float_inputs takes F,CLIP[,sr][,pack2|pack4]")
    codec = (int(parts[0]), float(parts[1]), "stochastic" if len(parts) == 3 else "nearest")
    return codec if pack is None else codec + (pack,)


def parse_round_bound(spec):
    """"TAIL" or "TAIL,ATTEMPTS" -> (tail, attempts), attempts 4 when left out; None, "" or a TAIL of 0 -> None."""
    if not spec:
        return None
    parts = [s.strip() for s in str(spec).split(",")]
    if len(parts) not in (1, 2):
        raise ValueError("--round_bound takes TAIL[,ATTEMPTS]")
    tail, attempts = float(parts[0]), int(parts[1]) if len(parts) == 2 else 4
    return (tail, attempts) if tail != 0.0 else None


def parse_dp_gauss(spec):
    """"SIGMA" or "SIGMA,TAIL" -> (sigma, tail), tail ceil(10 sigma) when left out; None, "" or a SIGMA of 0 -> None."""
    if not spec:
        return None
    from .. import dgauss
    parts = [s.strip() for s in str(spec).split(",")]
    try:
        if len(parts) not in (1, 2):
            raise ValueError
        sigma = float(parts[0])
        tail = int(parts[1]) if len(parts) == 2 else dgauss.default_tail(sigma)
    except ValueError:
        raise SystemExit("--dp_gauss takes SIGMA[,TAIL], TAIL an integer")
    return (sigma, tail) if sigma != 0.0 else None


def offline_schedule(n: int, iterations: int, always=(), dropout: float = 0.0) -> dict:
    """client id -> iterations in which it crashes before sending: `always` in every iteration, plus
    a fresh PCG64(seed=t).choice(n, round(dropout n), replace=False) set in each iteration t."""
    out = {i: set(range(1, iterations + 1)) for i in always}
    k = int(round(dropout * n))
    for t in range(1, iterations + 1):
        if k:
            for i in np.random.Generator(np.random.PCG64(t)).choice(n, k, replace=False):
                out.setdefault(int(i), set()).add(t)
    return out


def committee_dkg(num_clients: int, seed: int, latency: str = "cubic", gpu_dkg: bool = True) -> None:
    """The committee's key generation before the first iteration (protocol.configure(dkg=True)): a
    joint-Feldman DKG (abides/dkg) among the sorted committee, member index cnt + 1 as initialize
    assigns it, with as many coefficients as the default set-up's shamir_share(system_sk,
    max(1, committee_threshold), ...) call, so reconstruction and its Lagrange sets are untouched.
    The group key becomes the protocol's system_pk and each member's key share its committee_shared_sk."""
    from . import config_dkg
    from .dkg import keygen
    members = sorted(param.committee(num_clients))
    threshold = max(1, int(param.fraction * len(members)))
    keygen.configure(gpu_dkg=gpu_dkg)
    res = config_dkg.simulate(len(members), seed, latency=latency, poly_degree=threshold - 1)
    done = res["members"]
    if sorted(done) != list(range(1, len(members) + 1)):
        raise RuntimeError(f"{len(done)} of {len(members)} committee members finished the key generation")
    _, key = config_dkg.agreed(done)
    param.set_dkg_result(key, {cid: done[cnt + 1]["sk_share"] for cnt, cid in enumerate(members)})
    keygen.configure()


# Young-generation threshold for the run: the simulation allocates ~1.7 M container objects per
# iteration at n = 4096 (messages, payload dicts), and at CPython's default of 700 the resulting
# full collections over the agents' state took 5.7 s of a 67 s c5 event loop; at 50,000 they take
# 0.5 s and the loop 61.5 s (tools/probes/sim_gc_probe.py, profiles/r05_sim_gc_threshold.log).
GC_THRESHOLD0 = 50_000


def run(argv=None):
    ap, args = parse(argv)
    if args.config_help:
        ap.print_help()
        return None
    old_gc = gc.get_threshold()
    gc.set_threshold(max(old_gc[0], GC_THRESHOLD0), *old_gc[1:])
    try:
        return _run(args)
    finally:
        gc.set_threshold(*old_gc)


def _run(args):
    seed = args.seed or int(pd.Timestamp.now().timestamp() * 1000000) % (2**32 - 1)
    np.random.seed(seed)
    log.silent_mode = not args.verbose
    n = args.num_clients
    if not P.assert_power_of_two(n):
        raise ValueError("Number of clients must be power of 2")
    root = bytes.fromhex(args.root_seed_hex) if args.root_seed_hex else None
    if args.committee_size > args.num_clients:
        raise ValueError("committee_size cannot exceed num_clients")
    param.configure(root=root, L=args.vector_len, committee=args.committee_size,
                    gpu_deal=False if args.host_deal else None,
                    check_signatures=True if args.check_signatures else None,
                    gpu_verify=True if args.gpu_verify else None,
                    authenticate_shares=True if args.authenticate_shares else None,
                    dkg=True if args.dkg else None, codec=parse_float_inputs(args.float_inputs),
                    dp_noise=args.dp_noise, rotate=args.rotate, l2_clip=args.l2_clip,
                    round_bound=parse_round_bound(args.round_bound) or False,
                    dp_gauss=parse_dp_gauss(args.dp_gauss) or False, modular=args.modular or False)
    if param.dkg_on():
        committee_dkg(n, seed, args.latency, gpu_dkg=not args.host_dkg)
    offline = {int(x) for x in args.offline.split(",") if x.strip()}
    offline_its = offline_schedule(n, args.num_iterations, offline, args.dropout)
    print(f"Silent mode: {log.silent_mode}")
    print(f"Configuration seed: {seed}\n")

    start = pd.to_datetime("2023-01-01")
    stop = start + pd.to_timedelta("2000:00:00")
    default_delay = 1000000000 * 0.1
    kernel = Kernel("Base Kernel",
                    random_state=np.random.RandomState(seed=np.random.randint(low=0, high=2**32, dtype="uint64")))
    latency_rstate = np.random.RandomState(seed=np.random.randint(low=0, high=2**32, dtype="uint64"))
    agents = []
    t0 = time()
    for i in range(n):
        agents.append(ClientAgent(
            id=i, name=f"PPFL Client Agent {i}", type="ClientAgent", iterations=args.num_iterations, num_clients=n,
            neighborhood_size=args.neighborhood_size, debug_mode=args.debug_mode,
            random_state=np.random.RandomState(seed=np.random.randint(low=0, high=2**32, dtype="uint64")),
            offline_iterations=offline_its.get(i, ())))
    print(f"Client init took {timedelta(seconds=time() - t0)}")
    server = ServiceAgent(
        id=n, name="PPFL Service Agent", type="ServiceAgent",
        random_state=np.random.RandomState(seed=np.random.randint(low=0, high=2**32, dtype="uint64")),
        msg_fwd_delay=0, users=[*range(n)], iterations=args.num_iterations,
        round_time=pd.Timedelta(f"{args.round_time}s"), num_clients=n, neighborhood_size=args.neighborhood_size,
        parallel_mode=args.parallel_mode, debug_mode=args.debug_mode)
    agents.append(server)
    pairwise = (len(agents), len(agents))
    model_args = {"connected": True,
                  "min_latency": np.random.uniform(low=10000000, high=100000000, size=pairwise),
                  "jitter": 0.3, "jitter_clip": 0.05, "jitter_unit": 5}
    latency = LatencyModel(latency_model=args.latency, random_state=latency_rstate, kwargs=model_args)
    results = kernel.runner(agents=agents, startTime=start, stopTime=stop, agentLatencyModel=latency,
                            defaultComputationDelay=default_delay, skip_log=args.skip_log, log_dir=args.log_dir)
    print()
    print("######## Microbenchmarks ########")
    print(f"Protocol Iterations: {args.num_iterations}, Clients: {n}, ")
    print()
    print("Service Agent mean time per iteration (except setup)...")
    print(f"    Report step:         {results['srv_report']}")
    print(f"    Crosscheck step:     {results['srv_crosscheck']}")
    print(f"    Reconstruction step: {results['srv_reconstruction']}")
    print()
    print("Client Agent mean time per iteration (except setup)...")
    print(f"    Report step:         {results['clt_report'] / n}")
    print(f"    Crosscheck step:     {results['clt_crosscheck'] / param.committee_size}")
    print(f"    Reconstruction step: {results['clt_reconstruction'] / param.committee_size}")
    print()
    print("######## Known answer (all-ones inputs: final_sum == |U| in every slot) ########")
    for it in sorted(server.results):
        out, u = server.results[it], server.online_counts[it]
        gpu = server.gpu_ms.get(it, {})
        print(f"    iteration {it}: |U| = {u}, dropout pairs = {server.pairs_per_iteration.get(it, 0)}, "
              f"final_sum == |U| in every slot: {bool(np.all(out == u))}; report GPU {gpu.get('report', 0):.3f} ms, "
              f"unmask + D2H {gpu.get('reconstruction_unmask_gpu', 0):.3f} ms GPU "
              f"({gpu.get('reconstruction_unmask_wall', 0):.3f} ms wall)")
        if it in server.means:      # float inputs: the decoded mean against the mean of the clients' own floats
            exact = np.mean([np.asarray(agents[i].input_vector, np.float64) for i in server.online_ids[it]], axis=0)
            packed = f", {param.codec_pack()} per word" if param.codec_pack() > 1 else ""
            diff = server.means[it].astype(np.float64) - exact
            noised = ""
            if param.codec_noise_bits():    # the sum of |U| binomial shares: variance |U| b / 4, over (|U| 2^f)^2
                b, f = param.codec_noise_bits(), param.codec()[0]
                noised = (f", noise of {b} coins: standard deviation of the difference {float(np.std(diff)):.3e}, "
                          f"expected sqrt(|U| b) / (2 |U| 2^f) = {np.sqrt(u * b) / (2.0 * u * 2.0 ** f):.3e}")
            if param.dp_gauss() is not None:   # the sum of |U| table-sampled shares: |U| times the table's own variance
                from .. import dgauss
                (sigma, tail), f = param.dp_gauss(), param.codec()[0]
                var = float(dgauss.moments(param.dp_gauss_table())[1])
                noised = (f", discrete Gaussian noise sigma = {sigma:g}, tail = {tail}: standard deviation of the difference "
                          f"{float(np.std(diff)):.3e}, expected sqrt(|U| Var) / (|U| 2^f) = "
                          f"{np.sqrt(u * var) / (u * 2.0 ** f):.3e}")
            rotated = nonfinite = ""
            if param.rotate_bits():
                rotated = f", rotated in blocks of 2^{param.rotate_bits()}"
                nonfinite = f", {sum(agents[i].nonfinite for i in server.online_ids[it])} non-finite"
            scaled = ""
            if param.l2_clip() is not None:
                scaled = (f", {sum(agents[i].l2_factor < 1.0 for i in server.online_ids[it])} of {len(server.online_ids[it])} "
                          f"clients scaled to norm {param.l2_clip():g}")
                if param.round_bound() is not None:   # the sensitivity after rounding beside the one before it
                    redrawn = sum(agents[i].round_attempts[it] > 0 for i in server.online_ids[it])
                    scaled += (f", rounded within Delta = sqrt({server.round_max_sumsq}) / 2^{param.codec()[0]} = "
                               f"{float(np.sqrt(server.round_max_sumsq)) / 2.0 ** param.codec()[0]:g}, {redrawn} clients "
                               f"needed a redraw")
            modular = ""
            if param.modular() is not None:    # the near-wrap evidence the server kept, and the margin in noise deviations
                from .. import modular as M
                near, most = server.near_wrap[it]
                var = param.codec_noise_bits() / 4.0
                if param.dp_gauss() is not None:
                    from .. import dgauss
                    var = float(dgauss.moments(param.dp_gauss_table())[1])
                modular = (f", decoded modulo the field: H = {M.half_modulus(param.codec_pack())}, guard = {param.modular_guard()}, "
                           f"{near} sums at or beyond the guard, max |Qh| = {most}, margin (H - max |Qh|) / sqrt(|U| Var) = "
                           f"{M.margin_sigmas(param.codec_pack(), u, most, var):.3g} noise standard deviations (no probability)")
            print(f"    iteration {it}: float inputs {param.codec()}{packed}{rotated}: largest |final_mean - mean of the clients' floats| = "
                  f"{float(np.max(np.abs(diff))):.3e}{noised}, "
                  f"{sum(agents[i].clipped for i in server.online_ids[it])} elements clipped{nonfinite}{scaled}{modular}")
    print()
    results["server"] = server
    results["clients"] = agents[:n]
    return results
