from .base import BaseObserver  # noqa: F401
from .minmax import LSQObserver, MinMaxObserver  # noqa: F401
from .per_channel import PerChannelMinMaxObserver  # noqa: F401
from .percentile import PercentileObserver  # noqa: F401
from .mse import MSEObserver  # noqa: F401
from .per_channel_mse import PerChannelMSEObserver  # noqa: F401
from .per_group import PerGroupMinMaxObserver  # noqa: F401
