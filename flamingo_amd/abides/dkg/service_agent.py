"""DKG service agent (agent/dkg/SA_ServiceAgent.py surface): the members' bulletin board.

It computes nothing.  Each round it pools what the members sent and, at its wake-up, forwards it
(:166-261): after 1 s every dealer's share for member j and all commitments to member j
(SHARE_AND_COMMIT), 3 s later the complaints against each dealer to that dealer
(ACCEPT_OR_COMPLAIN), 2 s later the shares the dealers broadcast in answer (FORWARD_SHARE), and 2 s
later the QUAL sets the members reported (BCAST_QUAL), which ends the protocol.
"""
from __future__ import annotations

import pandas as pd

from ..agent import Agent
from ..message import Message


class SA_ServiceAgent(Agent):
    def __str__(self):
        return "[dkg server]"

    def __init__(self, id, name, type, random_state=None, msg_fwd_delay=1000000, num_clients=10, users=(), **_):
        super().__init__(id, name, type, random_state)
        self.users = list(users)
        self.num_clients = num_clients
        self.recv_users_shares, self.recv_users_commitments = {}, {}
        self.recv_users_complaints, self.recv_bcast_shares, self.recv_quals = {}, {}, {}
        self.users_shares, self.users_commitments = {}, {}
        self.users_complaints, self.bcast_shares, self.quals = {}, {}, {}
        self.current_iteration = 1
        self.current_round = 0
        self.sent = []       # (recipient, body) of everything forwarded, in order
        self.wake_times = []
        self.aggProcessingMap = {0: self.initFunc, 1: self.share_and_commit, 2: self.accept_or_complain,
                                 3: self.forward_share, 4: self.bcast_qual}

    def kernelStarting(self, startTime):
        self.setComputationDelay(0)
        super().kernelStarting(startTime)

    def wakeup(self, currentTime):
        super().wakeup(currentTime)
        self.wake_times.append(currentTime)
        self.aggProcessingMap[self.current_round](currentTime)

    def receiveMessage(self, currentTime, msg):
        super().receiveMessage(currentTime, msg)
        body = msg.body
        sender = body["sender"]
        if body["iteration"] != self.current_iteration:
            raise RuntimeError("wrong iteration number.")
        if body["msg"] == "share_and_commit":
            self.recv_users_shares[sender] = body["si_shares"]
            self.recv_users_commitments[sender] = body["commitments"]
        elif body["msg"] == "accept_or_complain":
            self.recv_users_complaints[sender] = body["complaints_towards"]
        elif body["msg"] == "forward_share":
            self.recv_bcast_shares[sender] = body["bcast_sij"]
        elif body["msg"] == "bcast_qual":
            self.recv_quals[sender] = body["qual"]

    def _forward(self, recipient, body, tag):
        self.sent.append((recipient, body))
        self.sendMessage(recipient, Message(body), tag=tag)

    # ------------------------------------------------------------ rounds
    def initFunc(self, currentTime):
        self.current_round = 1
        self.setWakeup(currentTime + pd.Timedelta("1s"))

    def share_and_commit(self, currentTime):
        self.users_shares, self.recv_users_shares = self.recv_users_shares, {}
        self.users_commitments, self.recv_users_commitments = self.recv_users_commitments, {}
        for j in self.users:
            self._forward(j, {"msg": "SHARE_AND_COMMIT",
                              "shares": {d: self.users_shares[d][j] for d in self.users_shares},
                              "commitments": self.users_commitments}, "server_share_and_commit")
        self.current_round = 2
        self.setWakeup(currentTime + pd.Timedelta("3s"))

    def accept_or_complain(self, currentTime):
        self.users_complaints, self.recv_users_complaints = self.recv_users_complaints, {}
        for d in self.users:
            self._forward(d, {"msg": "ACCEPT_OR_COMPLAIN",
                              "complaints_from": [j for j in self.users_complaints if d in self.users_complaints[j]]},
                          "server_accept_or_complain")
        self.current_round = 3
        self.setWakeup(currentTime + pd.Timedelta("2s"))

    def forward_share(self, currentTime):
        self.bcast_shares, self.recv_bcast_shares = self.recv_bcast_shares, {}
        for j in self.users:
            self._forward(j, {"msg": "FORWARD_SHARE", "bcast_shares": self.bcast_shares}, "server_forward_share")
        self.current_round = 4
        self.setWakeup(currentTime + pd.Timedelta("2s"))

    def bcast_qual(self, currentTime):
        self.quals, self.recv_quals = self.recv_quals, {}
        for j in self.users:
            self._forward(j, {"msg": "BCAST_QUAL", "output": self.quals}, "server_bcast_qual")
        self.current_round = 1
