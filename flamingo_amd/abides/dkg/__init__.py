"""Distributed key generation agents (agent/dkg surface): joint-Feldman DKG among the committee,
dealing and share checks batched on the MI355X engine."""
from .client_agent import SA_ClientAgent  # noqa: F401
from .service_agent import SA_ServiceAgent  # noqa: F401
