"""Every kernel launch goes through the launch helper of nmx_common.h (NMX_LAUNCH / NMX_LAUNCH_AS / NMX_LAUNCH_QUIET).

The name a launch reports (nmx_last_kernels) is the stringified kernel expression, and the opt-in to more than 64 KiB of
dynamic LDS belongs to the launch itself -- both hold only while no translation unit launches, opts in or notes a kernel
by hand.  Pure source check: reads py_neuromodulation_amd/csrc, builds and loads nothing.
"""

from __future__ import annotations

import re
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "py_neuromodulation_amd" / "csrc"
HELPER_HEADER = "nmx_common.h"
MACROS = ("NMX_LAUNCH_QUIET", "NMX_LAUNCH_AS", "NMX_LAUNCH")


def helper_line_numbers(lines: list[str]) -> dict[str, set[int]]:
    """Line indices of the helper's definition in nmx_common.h: the body of each NMX_LAUNCH* macro (its continuation lines)
    and the body of nmx_launch_allow_lds."""
    parts: dict[str, set[int]] = {}
    for name in MACROS:
        start = [i for i, ln in enumerate(lines) if re.match(rf"#define {name}\(", ln)]
        assert len(start) == 1, f"{name} is defined {len(start)} times"
        i = start[0]
        body = {i}
        while lines[i].rstrip().endswith("\\"):
            i += 1
            body.add(i)
        parts[name] = body
    start = [i for i, ln in enumerate(lines) if re.match(r"static inline void nmx_launch_allow_lds\(", ln)]
    assert len(start) == 1
    i = start[0]
    body = {i}
    while lines[i].rstrip() != "}":
        i += 1
        body.add(i)
    parts["nmx_launch_allow_lds"] = body
    return parts


def occurrences(token: str) -> list[tuple[str, int, str]]:
    """(file, line index, line) of every occurrence of `token` under csrc -- code, strings and comments alike."""
    out = []
    for path in sorted(CSRC.iterdir()):
        if not path.is_file():
            continue
        for i, ln in enumerate(path.read_text().splitlines()):
            if token in ln:
                out.append((path.name, i, ln))
    return out


def test_launches_opt_ins_and_notes_live_in_the_helper_only():
    parts = helper_line_numbers((CSRC / HELPER_HEADER).read_text().splitlines())

    def inside(hit, names):
        return hit[0] == HELPER_HEADER and any(hit[1] in parts[n] for n in names)

    launches = occurrences("hipLaunchKernelGGL")
    assert launches, "the helper launches through hipLaunchKernelGGL"
    stray = [h for h in launches if not inside(h, ("NMX_LAUNCH_QUIET",))]
    assert not stray, f"hipLaunchKernelGGL outside NMX_LAUNCH_QUIET: {stray}"

    opt_ins = occurrences("hipFuncSetAttribute")
    assert opt_ins, "the helper opts in through hipFuncSetAttribute"
    stray = [h for h in opt_ins if not inside(h, ("nmx_launch_allow_lds",))]
    assert not stray, f"hipFuncSetAttribute outside nmx_launch_allow_lds: {stray}"

    # the declaration (nmx_common.h) and the definition (nmx_api.hip) of nmxi_note_kernel are no calls
    notes = [h for h in occurrences("nmxi_note_kernel(") if not h[2].startswith('extern "C" void nmxi_note_kernel(const char* name)')]
    assert notes, "the override form notes the name it is given"
    stray = [h for h in notes if not inside(h, ("NMX_LAUNCH_AS",))]
    assert not stray, f"nmxi_note_kernel called outside NMX_LAUNCH_AS: {stray}"

    # NMX_LAUNCH reports through the override form, with the stringified kernel expression and nothing else
    body = "\n".join((CSRC / HELPER_HEADER).read_text().splitlines()[i] for i in sorted(parts["NMX_LAUNCH"]))
    assert "nmx_kern_name(#kern)" in body and "NMX_LAUNCH_AS(nmx_name_.s, kern," in body
    # ... and the override form and the quiet form launch through the one place that opts in
    body = "\n".join((CSRC / HELPER_HEADER).read_text().splitlines()[i] for i in sorted(parts["NMX_LAUNCH_AS"]))
    assert "NMX_LAUNCH_QUIET(kern," in body
    body = "\n".join((CSRC / HELPER_HEADER).read_text().splitlines()[i] for i in sorted(parts["NMX_LAUNCH_QUIET"]))
    assert body.index("nmx_launch_allow_lds(") < body.index("hipLaunchKernelGGL(")
