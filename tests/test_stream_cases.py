"""The list of ordering promises (tests/stream_cases.py) against include/tsdf_hip.h, and the figures DESIGN.md's "Streams and
events" quotes against the sources: a new entry point that takes a device pointer, or a changed ring, fails here until the list
and the document follow."""
import os
import re

import stream_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tsdf_hip.h")
CSRC = os.path.join(ROOT, "semantic_slam_amd", "csrc")


def declarations(header):
    """[(function, its parameter list, the comment in front of it)]: a comment belongs to every declaration that follows it up
    to the next comment that stands on lines of its own, as the header groups them."""
    src = open(header).read()
    out, comment = [], ""
    for m in re.finditer(r"(?P<c>^/\*.*?\*/)|(?P<d>^(?:int|int64_t|void|const char \*)\s*\**(?P<n>tsdf_[a-z0-9_]+)\s*\((?P<a>.*?)\)\s*;)", src,
                         flags=re.S | re.M):
        if m.group("c"):
            comment = m.group("c")
        else:
            out.append((m.group("n"), m.group("a"), comment))
    return out


def ordering_entry_points():
    """Functions with a device pointer among their parameters (a *_dev name; tsdf_copy_slices' destinations and the halos of the
    extractors may be device addresses), or under a comment that speaks of a stream or of waiting.  The whole of a grouped
    comment counts for every declaration under it: too many rather than too few."""
    names = set()
    for name, args, comment in declarations(HEADER):
        dev = re.search(r"_dev\b", args) or re.search(r"\b(tsdf_dst|weight_dst|halo_tsdf|halo_weight)\b", args)
        if dev or re.search(r"stream|wait|synchronous", comment, flags=re.I):
            names.add(name)
    return names


def test_parser_sees_the_whole_header():
    from test_abi import declared_functions
    assert sorted(n for n, _, _ in declarations(HEADER)) == declared_functions(HEADER)


def test_every_ordering_entry_point_is_listed_or_exempt():
    needed = ordering_entry_points()
    assert len(needed) > 40
    unaccounted = sorted(needed - set(sc.ORDERED) - set(sc.EXEMPT))
    assert not unaccounted, f"neither listed nor exempt: {unaccounted}"
    declared = {n for n, _, _ in declarations(HEADER)}
    assert set(sc.ORDERED) | set(sc.EXEMPT) <= declared, sorted((set(sc.ORDERED) | set(sc.EXEMPT)) - declared)
    assert not set(sc.ORDERED) & set(sc.EXEMPT), sorted(set(sc.ORDERED) & set(sc.EXEMPT))
    assert set(sc.ORDERED.values()) == sc.STREAMS
    assert all(len(why) > 20 for why in sc.EXEMPT.values())
    # every function with a caller's device pointer among its parameters makes a promise: none of them is exempt
    for name, args, _ in declarations(HEADER):
        if re.search(r"_dev\b", re.sub(r"\*\*\w+_dev\b", "", args)):     # (float **x_dev: an address the library returns)
            assert name in sc.ORDERED, name


def test_design_quotes_the_rings_as_they_are():
    capi = open(os.path.join(CSRC, "tsdf_capi.hip")).read()
    store = open(os.path.join(CSRC, "frame_store.h")).read()
    host = open(os.path.join(CSRC, "host_derive.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("#### Streams and events"):design.index("**What ships and what does not")]
    assert "constexpr int kStageSlots = 3;" in capi and "StageRing<Staged<tsdfk::RayVolume>, 1> ray;" in capi
    assert "3 rgb blocks" in section and "3 parameter blocks, 1 `RayVolume` block" in section and "3 pinned frames" in section
    assert "constexpr int kRingSlots = 4;" in store and "4 pinned frames (`kRingSlots`)" in section
    assert "constexpr int kBatchSideStreams = 4;" in host and "members < 8 ? 1 : kBatchSideStreams" in host
    assert "batch of 8 or more" in section and "`side[4]`" in section
