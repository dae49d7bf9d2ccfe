"""The import surface of the upstream Pano-NeRF tree that the zero-edit drop-in (pano_nerf_amd.install) has to live with, as
data for tests/test_dropin.py: which of its top-level directories are regular packages, which modules they hold, what
systems/base_system.py and systems/panonerf_system.py import from them, and the keyword arguments base_system.py builds the
model with (hparams key or local name per keyword).  Read with `ast` from a checkout of the upstream tree; stores names only.

    python tests/golden/make_dropin_golden.py <upstream checkout>   ->  tests/golden/dropin_layout.json
"""
import ast
import json
import os
import sys

PACKAGES = ("models", "utils", "datasets", "systems")
SYSTEMS = ("systems/base_system.py", "systems/panonerf_system.py")


def imports_of(tree):
    """[(module, [names])] of the `from <package>.x import ...` statements into the four packages, in source order."""
    out = []
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.module and node.module.split(".")[0] in PACKAGES:
            out.append((node.lineno, node.module, [a.name for a in node.names]))
    return [[m, names] for _, m, names in sorted(out)]


def model_kwargs(tree):
    """keyword -> {"hparam": key} | {"local": name} of the NeRFModel(...) call in BaseSystem.__init__."""
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "NeRFModel":
            kw = {}
            for k in node.keywords:
                v = k.value
                if isinstance(v, ast.Subscript) and isinstance(v.slice, ast.Constant):
                    kw[k.arg] = {"hparam": v.slice.value}
                elif isinstance(v, ast.Name):
                    kw[k.arg] = {"local": v.id}
                else:
                    raise ValueError(f"unexpected argument form for {k.arg}")
            return kw
    raise ValueError("no NeRFModel(...) call")


def density_channels(tree):
    """mlp_name -> num_density_channels of the if / elif chain in BaseSystem.__init__."""
    out = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.If) and isinstance(node.test, ast.Compare) and isinstance(node.test.comparators[0], ast.Constant):
            for st in node.body:
                if isinstance(st, ast.Assign) and st.targets[0].id == "num_density_channels":
                    out[node.test.comparators[0].value] = st.value.value
    return out


def main(ref):
    layout = {"packages": {}, "system_imports": {}}
    for p in PACKAGES:
        d = os.path.join(ref, p)
        layout["packages"][p] = {"regular": os.path.exists(os.path.join(d, "__init__.py")),
                                 "modules": sorted(f[:-3] for f in os.listdir(d) if f.endswith(".py") and f != "__init__.py")}
    for rel in SYSTEMS:
        tree = ast.parse(open(os.path.join(ref, rel)).read())
        layout["system_imports"][rel[:-3].replace("/", ".")] = imports_of(tree)
        if rel.endswith("base_system.py"):
            layout["model_kwargs"] = model_kwargs(tree)
            layout["num_density_channels"] = density_channels(tree)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin_layout.json")
    with open(out, "w") as f:
        json.dump(layout, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main(sys.argv[1])
