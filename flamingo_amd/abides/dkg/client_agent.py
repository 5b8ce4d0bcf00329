"""DKG committee member (agent/dkg/SA_ClientAgent.py surface).

Members are numbered 1..n, and member j's evaluation point is j (:41, :199-200).  On its wake-up a
member deals: a random polynomial of degree int(fraction n) + 1 (:42), its value at every member's
point and the commitments c_k G to its coefficients, sent to the server as `share_and_commit`
(:180-212).  The server's messages then drive three steps:

* SHARE_AND_COMMIT (:81-109): every dealer's share for this member and everybody's commitments.  All
  n shares are checked in one call (keygen.check_shares: one flm_feldman_verify launch, the grid
  form, x_bits = the bit length of n); the dealers whose share fails go into `accept_or_complain`.
* ACCEPT_OR_COMPLAIN (:111-129): the members that complained about this dealer; it answers with the
  shares it dealt them, `forward_share`, for everybody to see.
* FORWARD_SHARE (:131-157): every broadcast share is checked against its dealer's commitments at the
  complainer's point, in one more call (the row form, with a dealer array); a dealer with a
  broadcast share that fails is disqualified; `bcast_qual` reports the rest.
* BCAST_QUAL (:159-175): QUAL is the set most members reported, and the key share is
  sum_{i in QUAL} s_i(j) mod n.

Where this departs from the reference, on purpose: the reference hands verify_commitment the whole
dict of a dealer's broadcast shares (:145), which checks whatever sits under key 1 at the checking
member's own point; here each broadcast share is checked at the point of the member it was dealt to.
A member whose own complaint was answered by a share that verifies takes that share in place of the
one it refused (the reference keeps the refused one, :171, and would end with a wrong key share).
And each member also keeps the group key sum_{i in QUAL} C_{i,0}, which the reference never computes.
"""
from __future__ import annotations

import pandas as pd

from ..agent import Agent
from ..message import Message
from . import keygen
from .service_agent import SA_ServiceAgent as ServiceAgent
from ..flamingo.seeds import P256_N


class SA_ClientAgent(Agent):
    def __str__(self):
        return "[dkg member]"

    def __init__(self, id, name, type, num_clients=None, random_state=None, poly_degree=None, **_):
        super().__init__(id, name, type, random_state)
        self.users = list(range(1, num_clients + 1))
        # the reference's `threshold` (:42); --dkg under Flamingo passes the committee's own
        self.poly_degree = keygen.degree(num_clients) if poly_degree is None else int(poly_degree)
        self.prime = P256_N
        self.x_bits = max(1, num_clients.bit_length())
        self.recv_shares = {}
        self.recv_commitments = {}
        self.si_shares_with_recvrs = {}
        self.my_commitments = []
        self.sk_share = None
        self.group_key = None
        self.qual = None
        self.current_iteration = 1
        self.elapsed_time = {"CHECK": pd.Timedelta(0)}
        keygen.register_dealer(self)

    def kernelStarting(self, startTime):
        self.serviceAgentID = self.kernel.findAgentByType(ServiceAgent)
        self.setComputationDelay(0)
        super().kernelStarting(startTime + pd.Timedelta(self.random_state.randint(low=0, high=1000), unit="ns"))

    def wakeup(self, currentTime):
        super().wakeup(currentTime)
        self.sendShareCommitments()

    # ------------------------------------------------------------ dealing
    def shareCommitBody(self) -> dict:
        """The `share_and_commit` body: this dealer's share for every member and its commitments."""
        self.si_shares_with_recvrs, self.my_commitments = keygen.deal(self)
        return {"msg": "share_and_commit", "iteration": self.current_iteration, "sender": self.id,
                "si_shares": self.si_shares_with_recvrs, "commitments": self.my_commitments}

    def sendShareCommitments(self):
        self.sendMessage(self.serviceAgentID, Message(self.shareCommitBody()), tag="comm_key_generation")

    # ------------------------------------------------------------ the server's messages
    def receiveMessage(self, currentTime, msg):
        super().receiveMessage(currentTime, msg)
        body = msg.body
        if body["msg"] == "SHARE_AND_COMMIT":
            t0 = pd.Timestamp("now")
            self.recv_shares = dict(body["shares"])
            self.recv_commitments = body["commitments"]
            dealers = list(self.recv_shares)
            verdicts = keygen.check_shares([(self.recv_commitments[d], self.id, self.recv_shares[d][1])
                                            for d in dealers], x_bits=self.x_bits)
            complaints = [d for d, ok in zip(dealers, verdicts) if not ok]
            self.elapsed_time["CHECK"] += pd.Timestamp("now") - t0
            self.sendMessage(self.serviceAgentID,
                             Message({"msg": "accept_or_complain", "sender": self.id,
                                      "iteration": self.current_iteration, "complaints_towards": complaints}),
                             tag="comm_acc_compl")
        elif body["msg"] == "ACCEPT_OR_COMPLAIN":
            bcast = {j: self.si_shares_with_recvrs[j] for j in body["complaints_from"]}
            self.sendMessage(self.serviceAgentID,
                             Message({"msg": "forward_share", "sender": self.id,
                                      "iteration": self.current_iteration, "bcast_sij": bcast}),
                             tag="comm_acc_compl")
        elif body["msg"] == "FORWARD_SHARE":
            t0 = pd.Timestamp("now")
            rows = [(d, j, sij) for d, answered in body["bcast_shares"].items() if d in self.recv_commitments
                    for j, sij in answered.items()]
            verdicts = keygen.check_shares([(self.recv_commitments[d], j, sij[1]) for d, j, sij in rows],
                                           x_bits=self.x_bits)
            disqual = {d for (d, _, _), ok in zip(rows, verdicts) if not ok}
            for (d, j, sij), ok in zip(rows, verdicts):
                if ok and j == self.id:
                    self.recv_shares[d] = sij        # the share this member complained about, made good
            self.elapsed_time["CHECK"] += pd.Timestamp("now") - t0
            self.sendMessage(self.serviceAgentID,
                             Message({"msg": "bcast_qual", "sender": self.id, "iteration": self.current_iteration,
                                      "qual": set(self.recv_shares) - disqual}),
                             tag="comm_qual")
        elif body["msg"] == "BCAST_QUAL":
            quals = [frozenset(q) for q in body["output"].values()]
            agreed = max(quals, key=quals.count)
            self.qual = sorted(agreed)
            self.sk_share = sum(self.recv_shares[d][1] for d in self.qual) % self.prime
            self.group_key = keygen.group_key([self.recv_commitments[d][0] for d in self.qual])
            self.kernel.custom_state.setdefault("dkg", {})[self.id] = {
                "qual": self.qual, "sk_share": (self.id, self.sk_share), "group_key": self.group_key}
