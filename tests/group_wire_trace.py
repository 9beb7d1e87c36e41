"""The collectives of tests/test_group_wire.py's script on a DistShardGroup over gloo (world 2),
per step, as both ranks issued them: name, dtype[element count] (``all_gather`` with the
number of per-rank tensors).  Recorded from this project's own output before the group's
protocols were stated once; the wire format has not changed since, so neither has this table.
It is a literal on purpose: do not regenerate it from the code under test."""

STEPS = ("load", "read", "tick", "tick_no_events", "purge", "stats", "stats_two_edges", "compact",
         "compact_wrong_expect", "reclaim_all", "reclaim_slots", "reclaim_refused", "close")

HDR, HDRS = "broadcast int64[8]", "all_gather 2 x int64[8]"

TRACE = {
    "load": (HDR, "broadcast_object_list", "all_gather_object"),
    "read": (HDR, "broadcast_object_list", "all_gather_object"),
    # nine events, 25 bytes each; rank 1's orphans and evicted slots come back in the gather
    "tick": (HDR, "broadcast uint8[225]", "all_reduce uint8[2160]", HDRS, "gather uint8[64]"),
    "tick_no_events": (HDR, "all_reduce uint8[2048]", HDRS),
    "purge": (HDR, "all_reduce uint8[2048]", HDRS),
    "stats": (HDR, "all_gather 2 x int64[65]"),
    "stats_two_edges": (HDR, "broadcast float64[2]", "all_gather 2 x int64[65]"),
    "compact": (HDR, "all_reduce uint8[256]", HDRS, HDRS),
    "compact_wrong_expect": (HDR, "all_reduce uint8[256]", HDRS),
    "reclaim_all": (HDR, HDRS, HDRS, "gather uint8[84]"),
    "reclaim_slots": (HDR, "broadcast int32[2]", HDRS, HDRS),
    "reclaim_refused": (HDR, HDRS, "all_gather_object"),
    "close": (HDR,),
}
