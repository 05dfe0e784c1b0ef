"""Stand-in for the torchfcpe package (not installed here), which
rave/pitch_utils.py imports and calls at module level (:10-12) to load the
neural FCPE estimator onto a device.  The YIN half of that module needs none of
it: the stand-in hands back an object that refuses to infer."""


class _NoModel:
    def infer(self, *args, **kwargs):
        raise RuntimeError("torchfcpe stand-in: the FCPE model is not available")


def spawn_bundled_infer_model(device=None):
    return _NoModel()
