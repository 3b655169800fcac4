"""Rewrites tests/golden/scene_compile_digests.json from the built library: mi3pt_host_scene_compile on the scenes and configurations of
tests/test_scene_compile.py, and prints which fields of which rows changed against the file as it was.  Run it after a change that is MEANT to
change a buffer's bytes, and read the list: a field that was not meant to change is a finding, not a new golden value.

    python tests/golden/make_scene_compile_digests.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "webgpu-pathtracer_amd", "py"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from mi3pt_host import capi            # noqa: E402
import test_scene_compile as tsc       # noqa: E402


def main():
    with open(tsc.GOLDEN) as fh:
        old = json.load(fh)
    fields = list(capi.SCENE_COMPILE_FIELDS)
    new = {"fields": fields, "cases": {}}
    changed = {}
    for name, (nodes, tris) in tsc.scene_cases().items():
        rows = new["cases"][name] = {}
        for collapse, order, eight in tsc.CONFIGS:
            key = tsc.config_key(collapse, order, eight)
            got = capi.host_scene_compile(nodes, tris, collapse, order, bool(eight))
            rows[key] = [got[k] for k in fields]
            was = old["cases"].get(name, {}).get(key)
            for k, a, b in zip(fields, was or [None] * len(fields), rows[key]):
                if a != b:
                    changed.setdefault(k, []).append(f"{name} {key}")
    with open(tsc.GOLDEN, "w") as fh:
        fh.write(json.dumps(new, indent=0) + "\n")
    for k, rows in changed.items():
        print(f"{k}: {len(rows)} rows changed, e.g. {rows[0]}")
    if not changed:
        print("nothing changed")


if __name__ == "__main__":
    main()
