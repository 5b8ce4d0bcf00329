"""Flamingo client agent (agent/flamingo/SA_ClientAgent.py surface).

Per iteration the client (sendVectors, :198-348) finds its neighbours, draws
its self-mask seed m_i, Shamir-shares it to the committee (each share AES-GCM
encrypted under the ECDH key with that member, :214-244), derives a pairwise
seed per neighbour -- ECDH r_ij = a_i A_j -> SHA-256 -> key; h_ijt =
ChaCha20(key)(t) & 0xFFFF; H = hash_to_curve(h_ijt); s_ij = SHA-256(H)
(:253-292) -- ElGamal-encrypts H under the system key (:326-332, :434-447)
and sends the masked vector

    y_i = x_i + PRG(m_i) + sum_{j in N(i), j > i} PRG(s_ij) - sum_{j < i} PRG(s_ij)

(:304-324; x_i = all ones, :304).  GPU work: the mask expansion and
composition (MaskEngine.client_mask), every batch of P-256 scalar
multiplications (ECDH, ElGamal, decryption shares: MaskEngine.ec_mul_wire),
and the dealing and AES-GCM sealing of the m_i shares of all clients of an
iteration (protocol.mi_shares; the host path stays behind
protocol.configure(gpu_deal=False)).
Committee members sign the offline set (ECDSA, :351-368) and answer DEC with
sk_j * c0 for each dropout ciphertext plus their decrypted m_i shares
(:370-431).  With protocol.configure(check_signatures=True) they first verify
the server's signature and a quorum of the forwarded committee signatures
(signaturesHold: the check the reference leaves as a comment, :387).  With
protocol.configure(authenticate_shares=True) the m_i shares keep the AES-GCM
tag the reference drops (:242), bound to (iteration, dealer, member), and a
member whose shares do not all verify (openShares) sends TAG_CHECK_FAILED
instead of its shares.
"""
from __future__ import annotations

import logging

import numpy as np
import pandas as pd

from ... import crypto as C
from ..agent import Agent
from ..message import Message
from . import protocol as param
from . import wire
from .seeds import P256_N, shamir_share
from .service_agent import SA_ServiceAgent as ServiceAgent

_MASK128 = (1 << 128) - 1



def pair_prf(engine, keys, iteration: int) -> list:
    """h_ijt for every pair key r_ij, as the decimal strings the client hashes to the curve
    (SA_ClientAgent.py:276-283): str(int.from_bytes(ChaCha20(r_ij, nonce).encrypt(t.to_bytes(16,
    'big'))[0:4], 'big') & 0xFFFF).  Bytes 0-3 of that ciphertext are keystream word 0 XOR t's
    first four bytes, so one batched GPU PRG call over all keys gives them: PRG word 0 of a key is
    LE32(keystream[0:4]) ^ "abcd" (util/param.py:12,32)."""
    if not keys:
        return []
    rnd = int(iteration).to_bytes(16, "big")[:4]
    w = np.asarray(engine.prg_expand(list(keys), 1))[:, 0].astype(np.uint32) ^ np.uint32(0x64636261)
    # ciphertext byte k = keystream byte k (LE byte k of word 0) ^ rnd[k]; h = bytes 2..3, big endian
    b2 = ((w >> np.uint32(16)) & np.uint32(0xFF)) ^ np.uint32(rnd[2])
    b3 = ((w >> np.uint32(24)) & np.uint32(0xFF)) ^ np.uint32(rnd[3])
    return [str(v) for v in ((b2 << np.uint32(8)) | b3).tolist()]

class SA_ClientAgent(Agent):
    def __str__(self):
        return "[client]"

    def __init__(self, id, name, type, iterations=4, key_length=32, num_clients=128, neighborhood_size=1,
                 debug_mode=0, random_state=None, offline_iterations=()):
        super().__init__(id, name, type, random_state)
        self.logger = logging.getLogger(__name__)
        self.logger.setLevel(logging.INFO)
        if debug_mode:
            logging.basicConfig()
        self.num_clients = num_clients
        self.neighborhood_size = neighborhood_size
        self.vector_len = param.vector_len
        self.vector_dtype = param.vector_type
        self.prime = P256_N
        self.key_length = key_length
        self.neighbors_list = set()
        self.cipher_stored = None
        self.signed_payload = None   # what this member signed in the current iteration (signSendLabels)
        self.user_committee = param.committee(self.num_clients)
        self.committee_shared_sk = None
        self.committee_member_idx = None
        self.elapsed_time = {"REPORT": pd.Timedelta(0), "CROSSCHECK": pd.Timedelta(0),
                             "RECONSTRUCTION": pd.Timedelta(0)}
        self.no_of_iterations = iterations
        self.current_iteration = 1
        self.current_base = 0
        self.setup_complete = False
        # iterations in which this client crashes before sending (explicit dropout injection;
        # in the reference dropouts only come from late messages)
        self.offline_iterations = set(offline_iterations)
        self.input_vector = None     # None -> all ones (:304); with float inputs: a synthetic float32 update
        self.clipped = 0             # float inputs: elements of the last update that were clipped
        self.nonfinite = 0           # ... and, with the rotation on, its non-finite elements (clipped then counts
                                     # rotated coordinates)
        self.l2_factor = None        # float inputs with --l2_clip: the factor the last update was scaled by (1.0: within
        self.l2_norm = None          # the norm), and the update's own L2 norm, sqrt of the library's sum of squares
        self.dither_seed = None      # float inputs, stochastic rounding: the last iteration's dither seed
        self.round_attempt = None    # ... with --round_bound: the overall index of the candidate seed that was accepted
        self.rounded_sumsq = None    # (0: the first drawn), and the rounded update's sum of squares under it
        self.round_attempts = {}     # ... iteration -> round_attempt, for the run's report
        self.noise_seed = None       # float inputs with --dp_noise or --dp_gauss: the last iteration's noise seed
        pki = param.pki(num_clients)
        self.secret_key = pki.client_sk[id]
        self.public_key = pki.client_pk[id]
        self.system_pk = pki.system_pk
        self.committee_keys = {}     # member -> AES key (a_i A_c).x mod 2^128 (:234-236)
        self.symmetric_keys = {}     # (committee members) client -> AES key (:86-91)
        param.register_client(self)
        if param.dkg_on() and param.dkg_share(id) is not None:
            # the committee generated the key itself: what COMMITTEE_SHARED_SK would carry
            self.committee_member_idx, share = param.dkg_share(id)
            self.committee_shared_sk = (self.committee_member_idx, share)
        if id in self.user_committee:
            ids = list(range(num_clients))
            self.symmetric_keys = self._aes_keys(ids)

    def kernelStarting(self, startTime):
        if self.id == 0:
            for k in ("clt_report", "clt_crosscheck", "clt_reconstruction"):
                self.kernel.custom_state[k] = pd.Timedelta(0)
        self.serviceAgentID = self.kernel.findAgentByType(ServiceAgent)
        self.setComputationDelay(0)
        super().kernelStarting(startTime + pd.Timedelta(self.random_state.randint(low=0, high=1000), unit="ns"))

    def kernelStopping(self):
        for k, cat in (("clt_report", "REPORT"), ("clt_crosscheck", "CROSSCHECK"),
                       ("clt_reconstruction", "RECONSTRUCTION")):
            self.kernel.custom_state[k] = self.kernel.custom_state.get(k, pd.Timedelta(0)) + \
                self.elapsed_time[cat] / self.no_of_iterations
        super().kernelStopping()

    def wakeup(self, currentTime):
        super().wakeup(currentTime)
        self.sendVectors(currentTime)

    def receiveMessage(self, currentTime, msg):
        super().receiveMessage(currentTime, msg)
        body = msg.body
        if body["msg"] == "COMMITTEE_SHARED_SK":
            self.committee_shared_sk = body["sk_share"]
            self.committee_member_idx = body["committee_member_idx"]
        elif body["msg"] == "SIGN":
            if body["iteration"] == self.current_iteration:
                t0 = pd.Timestamp("now")
                self.cipher_stored = msg
                self.signSendLabels(currentTime, body["labels"])
                self.recordTime(t0, "CROSSCHECK")
        elif body["msg"] == "DEC":
            if body["iteration"] == self.current_iteration:
                t0 = pd.Timestamp("now")
                if self.cipher_stored is not None and self.cipher_stored.body["iteration"] == self.current_iteration:
                    b = self.cipher_stored.body
                    if not param.check_signatures_on() or self.signaturesHold(b["labels"], body["labels"]):
                        self.decryptSendShares(b["dec_target_pairwise"], b["dec_target_mi"], b["client_id_list"])
                self.cipher_stored = None
                self.signed_payload = None
                self.recordTime(t0, "RECONSTRUCTION")
        elif body["msg"] == "REQ" and self.current_iteration != 0:
            self.current_iteration += 1
            if self.current_iteration > self.no_of_iterations:
                return
            t0 = pd.Timestamp("now")
            self.sendVectors(currentTime)
            self.recordTime(t0, "REPORT")

    # --------------------------------------------------------------- round
    def _aes_keys(self, ids) -> dict:
        """(a_i A_j).x mod 2^128 per client j (:234-236, :86-91); the ECDH points of every
        client x committee pair come from one GPU batch (protocol.prefetch_committee_ecdh)."""
        param.prefetch_committee_ecdh(self.num_clients)
        return {j: (int.from_bytes(param.ecdh_wire(self.num_clients, self.id, j)[:32], "big") & _MASK128)
                .to_bytes(16, "big") for j in ids}

    def _rand_scalar(self) -> int:
        return int.from_bytes(bytes(self.random_state.randint(0, 256, size=32, dtype=np.uint8)), "big") % P256_N

    def sendVectors(self, currentTime):
        if self.current_iteration in self.offline_iterations:
            self.logger.info(f"client {self.id} is offline in iteration {self.current_iteration}")
            return
        self.neighbors_list = param.find_neighbors(param.root_seed, self.current_iteration, self.num_clients,
                                                   self.id, self.neighborhood_size)
        nb = list(self.neighbors_list)          # the reference's set order (:256, :295, :330)
        if self.id in self.neighbors_list:
            raise RuntimeError("id itself appears in its neighbor list")
        committee = sorted(self.user_committee)
        # the ECDH keys r_ij = SHA-256(a_i A_j) of the whole iteration's graph: one GPU batch, cached in
        # the protocol (pair_material below)
        if not self.committee_keys:
            self.committee_keys = self._aes_keys(committee)

        # m_i, its Shamir shares, one AES-GCM ciphertext per committee member (:214-244)
        # GPU path: the draws happen here all the same (protocol.mi_draw, the host path's order), and
        # the shares of every client of the iteration are dealt and sealed further down (mi_shares)
        gpu_deal = param.deal_on_gpu()
        mi_bytes = param.mi_draw(self, self.current_iteration)[0] if gpu_deal else \
            bytes(self.random_state.randint(0, 256, size=self.key_length, dtype=np.uint8))
        mi_number = int.from_bytes(mi_bytes, "big")
        threshold = int(param.fraction * len(self.user_committee))
        shares = [] if gpu_deal else shamir_share(mi_number, max(1, threshold), len(committee), self.prime,
                                                  rng=_PyRandom(self.random_state))
        enc_mi_shares = []
        for (_, y), cid in zip(shares, committee):
            nonce = bytes(self.random_state.randint(0, 256, size=16, dtype=np.uint8))
            if param.authenticate_shares_on():     # the tag the reference drops (:242), behind the ciphertext
                ct, tag = C.aes_gcm_seal(self.committee_keys[cid], y.to_bytes(self.key_length, "big"), nonce,
                                         param.share_aad(self.current_iteration, self.id, cid))
                ct += tag
            else:
                ct, _ = C.aes_gcm_encrypt(self.committee_keys[cid], y.to_bytes(self.key_length, "big"), nonce)
            enc_mi_shares.append((ct, nonce))

        # pairwise seeds: h_ijt -> H (group element) -> s_ij (:266-292), every client's in a few
        # batched launches (protocol.pair_material: one PRG launch for all h_ijt, the hash-to-curve table)
        pnb, _, _, s_ij = param.pair_material(self.current_iteration, self.num_clients,
                                              self.neighborhood_size)[self.id]
        if pnb != nb:
            raise RuntimeError("pair material built for another neighbour order")
        seeds = [mi_bytes] + [s[: self.key_length] for s in s_ij]
        signs = [1] + [1 if self.id < j else -1 for j in nb]

        # ElGamal under the system key: c0 = rG, c1 = H + r pk (:326-332, :434-447); every client's
        # r G and H + r pk of the iteration come from two GPU launches (protocol.elgamal_masks)
        _, rg, c1w = param.elgamal_masks(self, self.current_iteration, nb)
        c0 = C.points_from_wire(rg) if nb else []
        c1 = C.points_from_wire(c1w) if nb else []
        cipher = {(self.id, j): (c0[k], c1[k]) for k, j in enumerate(nb)}
        if gpu_deal:      # after elgamal_masks: every client's r's are drawn before the batch draws for it
            enc_mi_shares = param.mi_shares(self, self.current_iteration)

        codec = param.codec()
        if codec is None:
            x = None if self.input_vector is None else np.asarray(self.input_vector, np.uint32)[None, :]
            vec = param.engine().client_mask(np.array([0, len(seeds)], np.int64), seeds, signs, self.vector_len, x=x)[0]
        else:
            # float inputs ("replace it with model weights", :300-304): the fixed-point encoding is fused into
            # the masking, the VECTOR body is the same uint32 row.  The dither seed is this client's last draw.
            frac_bits, clip, rounding = codec
            if self.input_vector is None:
                from ...synthetic import float_update
                self.input_vector = float_update(self.id, self.vector_len, clip, param.rotate_bits())
            x = np.asarray(self.input_vector, np.float32)[None, :]
            L = self.vector_len
            norm = param.l2_clip()    # the update scaled to an L2 norm of at most this: before the rotation, or with it
            if norm is not None and not param.rotate_bits():
                x, factors, sumsq = param.engine().l2_clip(x, norm)
                self.l2_factor, self.l2_norm = float(factors[0]), float(np.sqrt(sumsq[0]))
            if param.rotate_bits():   # the iteration's public rotation in front of the encode; the clip bounds its output
                key = param.rotation_key(self.current_iteration)
                if norm is None:
                    x, nonfinite = param.engine().rotate(x, key, param.rotate_bits(), return_nonfinite=True)
                else:
                    x, nonfinite, factors, sumsq = param.engine().rotate(x, key, param.rotate_bits(), return_nonfinite=True,
                                                                         clip_norm=norm)
                    self.l2_factor, self.l2_norm = float(factors[0]), float(np.sqrt(sumsq[0]))
                L, self.nonfinite = param.rotated_len(), int(nonfinite[0])
            bound = param.round_bound()
            if bound is None:
                dither = [bytes(self.random_state.randint(0, 256, size=32, dtype=np.uint8))] \
                    if rounding == "stochastic" else None
            else:
                # conditional rounding: batches of candidate seeds where the one seed is drawn, the first whose rounded
                # row keeps its sum of squares within the bound is the dither seed; a row outside it is never sent
                attempts, max_sumsq = bound[1], param.round_max_sumsq()
                dither = None
                for batch in range(param.ROUND_BATCHES):
                    cands = self.random_state.randint(0, 256, size=(1, attempts, 32), dtype=np.uint8)
                    picked, chosen, sumsq = param.engine().round_select(x, frac_bits, clip, cands, max_sumsq)
                    if int(chosen[0]) < attempts:
                        dither = [picked[0].tobytes()]
                        self.round_attempt = batch * attempts + int(chosen[0])
                        self.rounded_sumsq = int(sumsq[0, int(chosen[0])])
                        self.round_attempts[self.current_iteration] = self.round_attempt
                        break
                if dither is None:
                    raise RuntimeError(f"client {self.id}: none of {param.ROUND_BATCHES * attempts} dither seeds kept the "
                                       f"rounded update's sum of squares within {max_sumsq}")
            seg = np.array([0, len(seeds)], np.int64)
            noise_bits = param.codec_noise_bits()
            if noise_bits:   # distributed DP: the noise seed is drawn after every other draw, the dither seed included
                self.noise_seed = bytes(self.random_state.randint(0, 256, size=32, dtype=np.uint8))
                vec, clipped = param.engine().client_encode_noise_mask(seg, seeds, signs, L, x, frac_bits,
                                                                       clip, param.codec_pack(), dither=dither,
                                                                       noise_bits=noise_bits, noise=[self.noise_seed],
                                                                       return_clipped=True)
            elif param.dp_gauss() is not None:   # the discrete Gaussian share: the same one draw, the table built in configure
                self.noise_seed = bytes(self.random_state.randint(0, 256, size=32, dtype=np.uint8))
                vec, clipped = param.engine().client_encode_gauss_mask(seg, seeds, signs, L, x, frac_bits, clip,
                                                                       param.dp_gauss_table(), [self.noise_seed],
                                                                       pack=param.codec_pack(), dither=dither,
                                                                       return_clipped=True)
            elif param.codec_pack() == 1:
                vec, clipped = param.engine().client_encode_mask(seg, seeds, signs, L, x, frac_bits, clip,
                                                                 dither=dither, return_clipped=True)
            else:   # packed: the body is param.ring_len() words, the masks with it
                vec, clipped = param.engine().client_encode_pack_mask(seg, seeds, signs, L, x, frac_bits,
                                                                      clip, param.codec_pack(), dither=dither,
                                                                      return_clipped=True)
            vec, self.clipped = vec[0], int(clipped[0])
            self.dither_seed = dither[0] if dither else None
        self.sendMessage(self.serviceAgentID, Message({
            "msg": "VECTOR", "iteration": self.current_iteration, "sender": self.id, "vector": vec,
            "enc_mi_shares": wire.serialize_tuples_bytes(enc_mi_shares),
            "enc_pairwise": wire.serialize_dim1_elgamal(cipher)}),
            tag="comm_key_generation")

    def signSendLabels(self, currentTime, msg_to_sign):
        payload = repr(msg_to_sign).encode()          # the reference signs dill.dumps(msg) (:352-356)
        self.signed_payload = payload
        sig = C.ecdsa_sign(self.secret_key, self.public_key, payload)
        self.sendMessage(self.serviceAgentID, Message({
            "msg": "SIGN", "iteration": self.current_iteration, "sender": self.id,
            "signed_labels": (payload, sig), "committee_member_idx": self.committee_member_idx}),
            tag="comm_sign_client")

    def signaturesHold(self, server_labels, dec_labels) -> bool:
        """The check the reference leaves as `# CHECK SIGNATURES` (:387), behind
        protocol.configure(check_signatures=True): the server's signature over the offline set this
        member was shown, and a quorum of committee signatures over the very payload it signed
        itself -- so a server that shows different offline sets to different decryptors gets no
        shares from them.  One batched verification per DEC (protocol.check_dec_signatures).  A
        member that refuses says so and sends no shares; the server's threshold check then decides."""
        server_ok, valid, needed = param.check_dec_signatures(self.num_clients, server_labels, dec_labels,
                                                              self.signed_payload)
        if server_ok and valid >= needed:
            return True
        self.logger.info(f"client {self.id}: signature check failed in iteration {self.current_iteration} "
                         f"(server {'ok' if server_ok else 'BAD'}, {valid} of {needed} committee signatures)")
        self.sendMessage(self.serviceAgentID, Message({
            "msg": "SIG_CHECK_FAILED", "iteration": self.current_iteration, "sender": self.id,
            "valid": valid, "needed": needed}), tag="sig_check_failed")
        return False

    def decryptSendShares(self, dec_target_pairwise, dec_target_mi, client_id_list):
        """dec_target_pairwise: serialize_dim1_elgamal JSON; dec_target_mi: serialize_tuples_bytes JSON."""
        if self.committee_shared_sk is None:
            self.sendMessage(self.serviceAgentID, Message({
                "msg": "NO_SK_SHARE", "iteration": self.current_iteration, "sender": self.id,
                "shared_result": None, "committee_member_idx": None}), tag="no_sk_share")
            return
        # sk_j * c0 for every dropout ciphertext (:393-400), one GPU batch
        _, c0w, _ = wire.elgamal_json_to_wire(dec_target_pairwise)
        sk = self.committee_shared_sk[1]
        dec_w, _ = param.engine().ec_mul_wire(c0w, C.scalars_to_wire([sk] * c0w.shape[0]))
        # decrypt this member's m_i shares (:402-420): one GPU launch for all of them, or one
        # OpenSSL context each on the host path
        sealed = list(zip(client_id_list, wire.deserialize_tuples_bytes(dec_target_mi)))
        if param.authenticate_shares_on():
            dec_mi, bad = self.openShares(sealed)
            if bad:
                self.logger.info(f"client {self.id}: tag check failed in iteration {self.current_iteration} "
                                 f"for the shares of {bad}")
                self.sendMessage(self.serviceAgentID, Message({
                    "msg": "TAG_CHECK_FAILED", "iteration": self.current_iteration, "sender": self.id,
                    "bad": bad}), tag="tag_check_failed")
                return
        elif sealed and param.deal_on_gpu():
            if len({(len(ct), len(nonce)) for _, (ct, nonce) in sealed}) != 1:
                raise RuntimeError("m_i share ciphertexts of one DEC differ in length")
            as_rows = lambda parts: np.frombuffer(b"".join(parts), np.uint8).reshape(len(sealed), -1)  # noqa: E731
            opened = param.engine().aes_gcm_xor_wire(as_rows(self.symmetric_keys[cid] for cid, _ in sealed),
                                                     as_rows(nonce for _, (_, nonce) in sealed),
                                                     as_rows(ct for _, (ct, _) in sealed))
            dec_mi = [int.from_bytes(row.tobytes(), "big") for row in opened]
        else:
            dec_mi = [int.from_bytes(C.aes_gcm_decrypt(self.symmetric_keys[cid], ct, nonce), "big")
                      for cid, (ct, nonce) in sealed]
        self.sendMessage(self.serviceAgentID, Message({
            "msg": "SHARED_RESULT", "iteration": self.current_iteration, "sender": self.id,
            "shared_result_pairwise": wire.wire_to_ecp_json(dec_w),
            "shared_result_mi": wire.serialize_dim1_list(dec_mi),
            "committee_member_idx": self.committee_member_idx}), tag="comm_secret_sharing")

    def openShares(self, sealed) -> tuple:
        """protocol.configure(authenticate_shares=True): open this member's (dealer, (ciphertext ||
        tag, nonce)) rows under the AAD the dealer sealed them with (protocol.share_aad) -- one
        flm_aes_gcm_open launch, or crypto.aes_gcm_open per row on the host path.  Returns (the
        shares in order, the dealers whose tag failed); a field of another length than 32 + 16
        bytes, or a nonce of another than 16, is a failed tag.  One bad ciphertext silences this
        member for the iteration (the server combines every client's m_i with one Lagrange set);
        it says so and the server's threshold check decides."""
        width = self.key_length + param.SHARE_TAG_LEN
        good = [k for k, (_, (ct, nonce)) in enumerate(sealed) if len(ct) == width and len(nonce) == 16]
        bad = [cid for cid, (ct, nonce) in sealed if len(ct) != width or len(nonce) != 16]
        rows = [sealed[k] for k in good]
        aads = [param.share_aad(self.current_iteration, cid, self.id) for cid, _ in rows]
        if rows and param.deal_on_gpu():
            as_rows = lambda parts: np.frombuffer(b"".join(parts), np.uint8).reshape(len(rows), -1)  # noqa: E731
            field = as_rows(ct for _, (ct, _) in rows)
            opened, ok = param.engine().aes_gcm_open_wire(as_rows(self.symmetric_keys[cid] for cid, _ in rows),
                                                          as_rows(nonce for _, (_, nonce) in rows),
                                                          field[:, :self.key_length], field[:, self.key_length:],
                                                          aad=as_rows(aads))
            plain = [row.tobytes() if v else None for row, v in zip(opened, ok)]
        else:
            plain = [C.aes_gcm_open(self.symmetric_keys[cid], ct[:self.key_length], ct[self.key_length:], nonce, aad)
                     for (cid, (ct, nonce)), aad in zip(rows, aads)]
        bad += [cid for (cid, _), p in zip(rows, plain) if p is None]
        return [int.from_bytes(p, "big") for p in plain if p is not None], sorted(bad)

    def recordTime(self, startTime, categoryName):
        self.elapsed_time[categoryName] += pd.Timestamp("now") - startTime

    def agent_print(*args, **kwargs):
        print(*args, **kwargs)


class _PyRandom:
    """randrange() over a numpy RandomState, so share polynomials follow the agent's seed."""

    def __init__(self, rs):
        self.rs = rs

    def randrange(self, n):
        return int.from_bytes(bytes(self.rs.randint(0, 256, size=40, dtype=np.uint8)), "big") % n
