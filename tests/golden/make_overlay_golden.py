"""What tests/test_overlay.py needs to know about a FollowMyHold checkout, recorded from the REFERENCE itself.

    python tests/golden/make_overlay_golden.py /path/to/FollowMyHold [output directory]

Writes ref_overlay.json: the module files of the checkout's src/foho (the layout the overlay must keep visible), where
each name `foho.configs` exports is defined, the directory the orchestrator puts first on every stage's PYTHONPATH
(main.py `_foho_src()`, relative to the checkout) and the orchestrator's own command lines for the three stages this
repository provides (main.py `_cmd`, with this repository's stage flags).  Nothing from the reference is copied: the
outputs are data.  The reference's OptimizationConfig values are fixture f7 of ref_meta.json (make_golden.py).
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

GUIDANCE_FLAGS = ["project_root", "cropped_obj_img_dir", "mask_dir", "moge_out_dir", "hunyuan_hoi_mesh_dir", "hamer_out_dir",
                  "h2m_rt_dir", "aligned_mano_dir", "guidance_out_dir"]


def main():
    co = os.path.abspath(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else HERE
    src = os.path.join(co, "src")
    pkg = os.path.join(src, "foho")
    modules = sorted(os.path.relpath(os.path.join(d, f), pkg) for d, _, fs in os.walk(pkg) for f in fs
                     if f.endswith(".py") and "__pycache__" not in d)
    # the stage flags are this repository's; import them before the checkout's package can shadow it
    sys.path.insert(0, ROOT)
    from foho.alignment import h2m, mano
    flags = {"foho.alignment.h2m": list(h2m.FLAGS), "foho.alignment.mano": list(mano.FLAGS)}
    for m in [k for k in sys.modules if k == "foho" or k.startswith("foho.")]:
        del sys.modules[m]
    sys.path[0] = src
    import foho.configs as C
    import foho.main as MAIN
    cmds = {"foho.guidance.run": MAIN._cmd("foho.guidance.run", {n: f"/data/my dir/{n}" for n in GUIDANCE_FLAGS})}
    for mod, fl in flags.items():
        cmds[mod] = MAIN._cmd(mod, {n: "/x/" + n for n in fl})
    rec = {"modules": modules,
           "configs_exports": {n: getattr(C, n).__module__ for n in C.__all__},
           "foho_src": os.path.relpath(MAIN._foho_src(), co),
           "guidance_flags": GUIDANCE_FLAGS, "stage_flags": flags, "commands": cmds}
    with open(os.path.join(out, "ref_overlay.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
