"""The slot cache of pkg/maps/lbmap/bpfservice.go, restated: which backend sits
in which slave slot of a service, so that scaling a service up or down moves
no backend to another slot (a flow's conntrack entry names its slave slot).

``BpfService.add_backend`` / ``delete_backend`` and ``LBMapCache.prepare_update``
follow addBackend / deleteBackend / prepareUpdate statement by statement,
including the sharing the Go code has: deleteBackend puts *one* fill record
into every slot it frees, and addBackend fills a hole by writing into the
record it finds there, so two holes freed by one deleteBackend change together.

Where the reference's choice hangs on Go's map iteration order, the rule here is:

* the fill backend is the remaining one with the fewest slots, a tie going to
  the one whose lowest slot index is smallest;
* delete_backend visits the slots in index order, so the holes it makes are
  queued in that order;
* prepare_update deletes the backends that went away in the order they were
  first added.

A backend is ``Backend(addr, port, rev_nat, weight)``; its id is the reference's
``ServiceValue.String()``: address, port and RevNat id (not the weight).
"""
from __future__ import annotations

import ipaddress
from typing import NamedTuple


class Backend(NamedTuple):
    addr: str
    port: int  # host order
    rev_nat: int
    weight: int = 0

    @property
    def id(self) -> str:
        return f"{ipaddress.ip_address(self.addr)}:{self.port} ({self.rev_nat})"


class _Slot:
    """bpfBackend: shared by reference between the slots one deleteBackend freed."""

    def __init__(self, value: Backend, is_hole: bool = False):
        self.id, self.is_hole, self.value = value.id, is_hole, value


class BpfService:
    def __init__(self, frontend):
        self.frontend = frontend
        self.holes: list[int] = []
        self.by_index: dict[int, _Slot] = {}
        self.unique: dict[str, Backend] = {}

    def add_backend(self, b: Backend) -> None:
        if self.holes:
            index = self.holes.pop(0)
            slot = self.by_index[index]
            slot.value, slot.id, slot.is_hole = b, b.id, False
        else:
            self.by_index[len(self.unique) + 1] = _Slot(b)
        self.unique[b.id] = b

    def delete_backend(self, b: Backend) -> None:
        remove, dup, lowest = [], {}, {}
        for index in sorted(self.by_index):
            s = self.by_index[index]
            if s.id == b.id:
                remove.append(index)
            else:
                dup[s.id] = dup.get(s.id, 0) + 1
                lowest.setdefault(s.id, index)
        if not dup:
            self.holes, self.by_index = [], {}
        else:
            fill_id = min(dup, key=lambda i: (dup[i], lowest[i]))
            fill = _Slot(self.unique[fill_id], is_hole=True)
            for index in remove:
                if not self.by_index[index].is_hole:
                    self.holes.append(index)
                self.by_index[index] = fill
        self.unique.pop(b.id, None)

    def backends(self) -> list[Backend]:
        return [self.by_index[i].value for i in range(1, len(self.by_index) + 1)]


class LBMapCache:
    def __init__(self):
        self.entries: dict[str, BpfService] = {}

    def prepare_update(self, frontend_id: str, backends: list[Backend]) -> BpfService:
        svc = self.entries.setdefault(frontend_id, BpfService(frontend_id))
        new = {b.id for b in backends}
        for key in [k for k in svc.unique if k not in new]:
            svc.delete_backend(svc.unique[key])
        for b in backends:
            if b.id not in svc.unique:
                svc.add_backend(b)
        return svc

    def delete(self, frontend_id: str) -> None:
        self.entries.pop(frontend_id, None)
