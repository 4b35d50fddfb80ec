------------------------------ MODULE spin_flag_unfair ------------------------------
(* spin_flag with an unfair setter: the spinner may spin for ever (a real cycle Check -> Again -> Check). *)
EXTENDS Naturals

(* --algorithm spin_flag_unfair
variables flag = 0;

fair process Spinner = 0
begin
  Check: while flag = 0 do
    Again: skip;
  end while;
end process

process Setter = 1
begin
  Set: flag := 1;
end process

end algorithm *)
=============================================================================
