"""Scene assets that tests/conftest.py does not list: unpacked and checked the way conftest.scene_path does it
(per-user cache, sha256 of the reference's file, atomic rename).  Scenes conftest knows are passed on to it."""
import hashlib
import lzma
import os
import tempfile

import conftest

# sha256 of the reference's P3D_Scenes/<name>.p3f (see tests/golden/README.md)
EXTRA_SCENE_SHA256 = {
    # level-4 sphereflake: 7 381 spheres, one plane, three lights
    "balls_high": "8214c502ea38fe8009db844b3066fd8990aa3b38f0c56c45b583efc328811074",
}


def scene_path(name):
    """Unpack tests/golden/scenes/<name>.p3f.xz into a per-user cache and return the path."""
    if name in conftest.SCENE_SHA256:
        return conftest.scene_path(name)
    cache = os.path.join(tempfile.gettempdir(), "p3d_scene_cache_%d" % os.getuid())
    os.makedirs(cache, exist_ok=True)
    out = os.path.join(cache, name + ".p3f")
    if not os.path.exists(out):
        with lzma.open(os.path.join(conftest.GOLDEN, "scenes", name + ".p3f.xz"), "rb") as f:
            data = f.read()
        assert hashlib.sha256(data).hexdigest() == EXTRA_SCENE_SHA256[name], name
        tmp = out + ".%d.tmp" % os.getpid()
        with open(tmp, "wb") as f:
            f.write(data)
        os.replace(tmp, out)
    return out
