"""Records the routes of the six "stream form + tiled form" linear families (ao_mx_linear_route, ao_wo8_linear_route,
ao_fp8_block_linear_route, ao_fp8_block_grouped_mm_route, ao_nvfp4_linear_route, ao_nvfp4_grouped_mm_route) into
two_form_routes.json: host logic only, no GPU.  Run it with the library of the commit whose routes are to be pinned:

    python tests/golden/make_two_form_routes.py

The file holds the two grids (dense: every format under every ao_*_set_form value at M x N x K; grouped: the same at
M_total x N x K x E), the distinct seven-field routes it met (kernel, waves, m-tiles, tile rows, tile columns, grid x, grid y --
kernel 0: the family refuses the shape), and per "family/format/form" key the index of the route of every grid cell, M outermost
and K (grouped: E) innermost.  The route table only grows: a route the file already lists keeps its index, so regenerating the
file leaves the index lists of unchanged routes as they are.
tests/test_host_dispatch.py::test_two_form_routes_match_the_recording compares the built library against it.
"""
import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

FAMILIES = {  # family -> (route query, form override, {format name: the arguments in front of the shape}, grouped)
    "mx": ("ao_mx_linear_route", "ao_mx_linear_set_form", {"e4m3": (0,), "e2m1": (4,)}, False),
    "wo8": ("ao_wo8_linear_route", "ao_wo8_linear_set_form", {"int8": (0,), "e4m3": (1,)}, False),
    "fp8_block": ("ao_fp8_block_linear_route", "ao_fp8_block_linear_set_form", {"e4m3": ()}, False),
    "fp8_block_grouped": ("ao_fp8_block_grouped_mm_route", "ao_fp8_block_grouped_mm_set_form", {"e4m3": ()}, True),
    "nvfp4": ("ao_nvfp4_linear_route", "ao_nvfp4_linear_set_form", {"wo": (0,), "dyn": (1,)}, False),
    "nvfp4_grouped": ("ao_nvfp4_grouped_mm_route", "ao_nvfp4_grouped_mm_set_form", {"wo": (0,), "dyn": (1,)}, True),
}
FORMS = (0, 1, 2)
M_GRID = (0, 1, 16, 17, 32, 33, 64, 65, 128, 129, 4194241)  # (4194241 rows at K <= 48: the grid-row cap of the forced stream form)
N_GRID = (1, 16, 17, 4096, 16400)
K_GRID = (16, 32, 48, 128, 160, 384, 4096)
# grouped (M_total, N, K, E): the mean-size seam on both sides, the refused E, the stream form's grid y = E, the tiled form's
# ceil(M_total / edge) + E and that sum passing 65535
GROUPED_GRID = ((0, 1, 16, 17, 64, 65, 129, 4194241), (1, 17, 4096), (16, 128, 384, 4096), (1, 8, 65535, 65536))


def grid(family):
    """The shapes of a family's cells, in the order of its index lists."""
    return list(itertools.product(*(GROUPED_GRID if FAMILIES[family][3] else (M_GRID, N_GRID, K_GRID))))


def route(lib, family, fmt, *shape):
    out = (ctypes.c_int32 * 7)()
    rc = getattr(lib, FAMILIES[family][0])(*FAMILIES[family][2][fmt], *shape, out, 7)
    assert rc == 0, rc
    return tuple(out)


def record_form(lib, family, form):
    """{"family/format/form": [route of every grid cell]} of one family under one forced form, restored to 0;
    form None: under whatever the calling thread has set, filed as form 0."""
    set_form, fmts = FAMILIES[family][1:3]
    try:
        if form is not None:
            assert getattr(lib, set_form)(form) == 0
        return {"%s/%s/%d" % (family, fmt, form or 0): [route(lib, family, fmt, *shape) for shape in grid(family)] for fmt in fmts}
    finally:
        if form is not None:
            getattr(lib, set_form)(0)


def record(lib):
    rec = {}
    for family in FAMILIES:
        for form in FORMS:
            rec.update(record_form(lib, family, form))
    return rec


def load_doc():
    with open(os.path.join(HERE, "two_form_routes.json")) as f:
        return json.load(f)


def load():
    doc = load_doc()
    assert (tuple(doc["M"]), tuple(doc["N"]), tuple(doc["K"])) == (M_GRID, N_GRID, K_GRID)
    assert tuple(tuple(doc["grouped"][axis]) for axis in ("M_total", "N", "K", "E")) == GROUPED_GRID
    routes = [tuple(r) for r in doc["routes"]]
    return {key: [routes[i] for i in idx] for key, idx in doc["cells"].items()}


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from ao_amd import _lib

    rec = record(_lib.lib())
    routes = [tuple(r) for r in load_doc()["routes"]] if os.path.exists(os.path.join(HERE, "two_form_routes.json")) else []
    routes += sorted({r for cells in rec.values() for r in cells} - set(routes))
    index = {r: i for i, r in enumerate(routes)}
    lines = ['{"M": %s, "N": %s, "K": %s,' % (json.dumps(M_GRID), json.dumps(N_GRID), json.dumps(K_GRID)),
             ' "grouped": {%s},' % ", ".join('"%s": %s' % (axis, json.dumps(values)) for axis, values in zip(("M_total", "N", "K", "E"), GROUPED_GRID)),
             ' "routes": [%s],' % ",\n  ".join(json.dumps(r) for r in routes), ' "cells": {']
    lines.append(",\n".join('  "%s": %s' % (key, json.dumps([index[r] for r in cells], separators=(",", ":"))) for key, cells in rec.items()))
    lines.append(" }}")
    with open(os.path.join(HERE, "two_form_routes.json"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d cells, %d distinct routes" % (sum(len(c) for c in rec.values()), len(routes)))
