"""Abstract inverter interface (reference null_inverter.py:5-15)."""


class NullInverter:
    def __init__(self, model):
        self.model = model

    def to(self, device):
        self.model.to(device)
        return self

    def invert(self, target_img, depth, prompt, num_inner_steps=10, early_stop_epsilon=1e-5, verbose=False):
        raise NotImplementedError("Null inverter must implement invert method.")

    def invert_batch(self, target_imgs, depths, prompts, num_inner_steps=10, early_stop_epsilon=1e-5, max_timesteps=None):
        """K images inverted one after the other through `invert` (not in the reference): one result per image, in input
        order.  Inverters that batch the work override this."""
        if not (len(target_imgs) == len(depths) == len(prompts)):
            raise ValueError("invert_batch: target_imgs, depths and prompts must have the same length")
        extra = {} if max_timesteps is None else {"max_timesteps": max_timesteps}
        return [self.invert(img, depth, prompt, num_inner_steps=num_inner_steps, early_stop_epsilon=early_stop_epsilon, **extra)
                for img, depth, prompt in zip(target_imgs, depths, prompts)]
