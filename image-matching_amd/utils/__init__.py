"""Mirror of the reference's `utils` package path: the helpers of the pseudo-label export that run in libimx."""
