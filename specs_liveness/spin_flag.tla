------------------------------ MODULE spin_flag ------------------------------
(* One process spins while flag = 0, a fair one sets the flag: Termination holds. *)
EXTENDS Naturals

(* --algorithm spin_flag
variables flag = 0;

fair process Spinner = 0
begin
  Check: while flag = 0 do
    Again: skip;
  end while;
end process

fair process Setter = 1
begin
  Set: flag := 1;
end process

end algorithm *)
=============================================================================
